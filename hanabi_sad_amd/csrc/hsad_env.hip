// hsad_env.hip — batched Hanabi environment for MI355X (gfx950): reset / step / observe for G
// concurrent games per launch.  Implements the hsad_env_* entry points of include/hsad.h.
//
// What it replaces (reference, all CPU): HanabiEnv::reset/step/computeFeatureAndLegalMove
// (cpp/hanabi_env.cc:9-205), rela::VectorEnv (rela/env.h:29-108) and the HLE engine + canonical
// encoder behind them.  Written from scratch for CDNA4; the algorithmic contract is the oracle's
// (oracle/hanabi_oracle.cc), the data structures are not:
//
//  * State lives in HBM as struct-of-arrays *planes* of packed u32 bit-fields, game index
//    fastest ([plane][G]) so a wavefront's 64 lanes (= 64 games) load/store each plane with one
//    coalesced 256-B access (which plane holds what, and the fields of every word: hsad_planes.h).  The per-game std::mt19937 is kept as 624 words per game and advanced
//    incrementally (one word regenerated per draw), so there is never a 624-word twist stall.
//  * One wavefront = 64 games.  State planes are staged in LDS ([plane][lane], conflict-free) so
//    the game logic can index hands/knowledge by a run-time seat without scratch spills.
//  * Observations are first built as *bit rows* in LDS (one ds_or per one-hot / thermometer
//    group), then the whole wavefront expands the 64 games' rows to fp32 with aligned, fully
//    coalesced 16-byte stores — the kernel is HBM-write bound by construction
//    (P*(F+A+3H+1)*4 B per game step).
//  * libstdc++'s discrete_distribution / generate_canonical / shuffle / uniform_int (Lemire)
//    are restated explicitly so trajectories are bit-identical to the oracle.

#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdlib>
#include <cstdio>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "hsad.h"
#include "hsad_deal_fast.h"
#include "hsad_obs_row.h"
#include "hsad_planes.h"

namespace {

constexpr int kWave = 64;
constexpr int kMtN = 624;
constexpr int kMtM = 397;

struct EnvParams {
  static constexpr bool kScripted = false;
  int G, Gpad, P, H, A, F, F0, LAL, OB, OD, OL, OK, DECKW;
  int max_len, sad, shuffle_color, bomb, kmode, n_eps, track_dh, npl;
  int nthreads;    // workgroup size: 128 (wave 0 logic, wave 1 LDS clearing, both build + stream) or 256 (two more waves for clearing,
                   // row building and streaming: when the launch has so few workgroups that a CU would hold only four waves)
  int gpw;         // games per workgroup: 64 (one per lane of the logic wave) or 32 (lanes 32-63 idle in the logic phase, half
                   // the LDS bit rows): twice the workgroups when 64-game ones would leave most CUs with a single one
  int obs_words, legal_words, own_words, win_w;
  int win_words;   // LDS words per lane of the mt19937 prefetch window: win_w when win_w <= 32 (old words stay in registers,
                   // only the regenerated ones are stored), 2 * win_w + 1 otherwise
  int seed0, deal_mode, nt_stores;
  int g_begin, g_count;            // launch covers games [g_begin, g_begin + g_count); g_begin % 64 == 0
  unsigned long long policy_seed;  // MODE 2 (step with built-in random-legal policy)
  int n_iter;       // MODE 3: iterations this launch runs for its games (persistent rollout; 1 otherwise)
  int delta;        // env_rollout_pipe_kernel: two copies of the observation bit rows in LDS; every stream of the launch but the first
                    // stores only the lines of priv_s whose bits changed since the stream before (rollout_delta_active).  Bit 0;
                    // bits 1 and 2 link the launches of one call (see phase below)
  int compact;      // with delta: the stream wave lists the changed units first and stores from the list (stream_bits_f32_compact):
                    // 1 = 128-byte lines, 2 = 64-byte half lines (hsad_env_set_rollout_unit)
  int stagger_ticks;  // MODE 3, n_iter > 1: workgroup b starts (b % 8) * stagger_ticks (100 MHz) late, see env_kernel
  int stagger_mode;   // which workgroups start late (developer switch HSAD_ENV_STAGGER_MODE, see env_rollout_kernel)
  int64_t* a_out;                  // MODE 2: where the sampled actions are recorded ([G,P] each)
  int64_t* g_out;
  uint32_t* planes;
  uint32_t* mt;
  const float* eps_list;
  uint8_t* deck_hist;
  uint32_t* err;
  uint32_t* act_count;
  unsigned long long* legal_bits;  // [G, P] compact legal-move masks (bit uid), side output for device consumers
  float* priv_s;
  float* legal;
  float* own;
  float* eps;
  // device-consumer outputs (hsad_env_bind_packed): the observation rows in the replay's stored format (bit words) and as the
  // net's bf16 GEMM operand, written from the same LDS bit rows; obs_f32 = 0 then skips the float32 observation stream
  unsigned long long* priv_bits;   // [G*P][pw64]
  unsigned long long* legal_out;   // [G*P]
  unsigned long long* own_bits;    // [G*P]
  unsigned short* priv16;          // [G*P][ld16] bf16, columns F..ld16-1 zero
  int pw64, ld16, obs_f32;
  unsigned dbg_units_hi;           // (see dbg_units_lo)
  float* reward;
  uint8_t* terminal;
  unsigned long long* dbg;  // optional wall_clock64 stamps of thread 0 at phase boundaries: [grid][8] (hsad_env_debug_timing), or per
                            // iteration of a persistent launch [grid][dbg_iters][16] (hsad_env_debug_trace; slot map: env_stamp)
  int dbg_iters;
  // optional, with the trace layout of dbg: the address of uint64 [grid][dbg_iters], the units of priv_s the stream wave stored for
  // the rows of `it - 1`, counted in the unit that stream decided by (hsad_env_debug_units); 0: off.  Kept as two halves in what
  // was padding behind dbg_iters and obs_f32, so that the struct keeps its size and every field its offset: a pointer appended to
  // the struct moves the later kernel arguments and changes the code of kernels that never read it (tools/isa_compare.py).
  unsigned dbg_units_lo;
  // phase lock of stream partitions (hsad_env_rollout_random with K > 1): partition p > 0 starts its launch `lock_ticks`
  // (10 ns units) after partition p-1 started the launch with the same tag, so that one partition's latency-bound logic
  // phase keeps overlapping the other's HBM stream.  Timing only: a bounded wait, results never depend on it.
  unsigned long long* phase;  // [16][2]: {tag, wall_clock64 at launch start} per partition, or NULL
  int part, n_part, lock_ticks;
  unsigned long long launch_tag, first_tag;   // first_tag: tag of the first iteration of this rollout call
  // The carry buffer of the chain of one call's persistent launches (hsad_env_set_rollout_chain) travels in `phase`, which only
  // partitioned launches (part >= 0, always one iteration) otherwise use, so that the struct keeps its size and every field its
  // offset (see dbg_units_lo).  In a launch of env_rollout_pipe_kernel with delta: phase = the env's carry buffer, uint32
  // [workgroups][obs_words], or NULL; delta bit 1 (kChainIn) = the buffer holds the rows the launch before streamed last,
  // bit 2 (kChainOut) = leave this launch's last rows there for the next one.  (The flags ride in delta because the loop of the
  // kernel reads that field anyway: a flag in a field of its own is one more value the kernel holds for the whole launch.)
  // pacing of a persistent launch (rollout_pace): every workgroup adds 1 to *pace at the top of each iteration, so the word says how
  // far the launch as a whole has come; a workgroup ahead of that mean delays its observation stream.  Timing only.
  unsigned long long* pace;        // the env's progress word, or NULL: no pacing (and no atomics) in this launch
  unsigned long long pace_base;    // value of *pace when this launch starts (host-tracked: no memset per launch)
  unsigned long long pace_inv_q32; // 2^32 / pace_blocks
  int pace_blocks;                 // workgroups of this launch that have games (and therefore count)
  int pace_l0_q8, pace_cap_ticks;  // dead band (iterations, 8 fractional bits) and cap of one delay (100 MHz ticks)
  // the game's rules (hsad_env_create_rules).  Read only by the variant instantiations (V = true); the full game's kernels
  // (V = false) compile them in as constants.  variant = 0 for 5 colours, 5 ranks, 8 information and 3 life tokens.
  int nC, nR, max_info, max_life, deck_max, variant;
  unsigned long long deck_full;    // the full deck's 2-bit card counts, type colour*5+rank (unused types 0)
};

// deal script of an env (hsad_env_rewind_scripted): cards [Gpad, 52] card types in deal order, count [Gpad] scripted deals per game
struct DealScript {
  uint8_t* cards;
  int32_t* count;
};
// What env_step_scripted_kernel takes instead of EnvParams.  The step path (env_body, env_logic, deal_one) is a template over its
// parameter struct and reads the script only where kScripted says so: EnvParams, and with it every kernel of an env that never
// received a script, is what it was before scripts existed.
struct ScriptedParams : EnvParams {
  static constexpr bool kScripted = true;
  DealScript sc;
};

constexpr uint32_t kIdentityPerm = (0u) | (1u << 3) | (2u << 6) | (3u << 9) | (4u << 12);
constexpr uint32_t kIdentityPermBoth = kIdentityPerm | (kIdentityPerm << 15);
// full deck: counts 3,2,2,2,1 per colour, 2 bits each
__host__ __device__ constexpr uint64_t full_deck_bits() {
  uint64_t d = 0;
  for (int c = 0; c < 5; ++c) {
    const int cnt[5] = {3, 2, 2, 2, 1};
    for (int r = 0; r < 5; ++r) d |= (uint64_t)cnt[r] << (2 * (c * 5 + r));
  }
  return d;
}

// deck of a variant: card instances 3 (rank 0), 1 (rank R-1), 2 otherwise; rank 0 is tested first (R = 1: 3 cards per colour)
__host__ __device__ constexpr uint64_t deck_bits(int C, int R) {
  uint64_t d = 0;
  for (int c = 0; c < C; ++c)
    for (int r = 0; r < R; ++r) d |= (uint64_t)(r == 0 ? 3 : (r == R - 1 ? 1 : 2)) << (2 * (c * 5 + r));
  return d;
}

// The game's rules as the kernels see them.  Card types keep the full game's colour*5+rank layout in every plane whatever C
// and R are (a variant's unused types simply count 0), so only the rules and the encoder's section geometry vary.  The full
// game's rules are static constants (FullRules: its kernels see literals, as before variants existed); a variant's are read
// from EnvParams (Rules).  Both are used as `ru.C` etc.
struct Rules {
  int C, R, MI, ML;    // colours, ranks, max information tokens, max life tokens
  int deck;            // MaxDeckSize
  uint64_t full;       // deck_bits(C, R)
  uint32_t cmask, rmask;  // plausible colours / ranks of a fresh card
  int CR, KS, DW;      // bits per card, knowledge stride per card (CR + C + R), discard thermometer width per colour
};
struct FullRules {
  static constexpr int C = 5, R = 5, MI = 8, ML = 3, deck = 50;
  static constexpr uint64_t full = full_deck_bits();
  static constexpr uint32_t cmask = 31u, rmask = 31u;
  static constexpr int CR = 25, KS = 35, DW = 10;
};
template <bool V>
struct RulesOf {
  static __device__ __forceinline__ FullRules make(const EnvParams&) { return FullRules{}; }
};
template <>
struct RulesOf<true> {
  static __device__ __forceinline__ Rules make(const EnvParams& ep) {
    const int C = ep.nC, R = ep.nR;
    return Rules{C, R, ep.max_info, ep.max_life, ep.deck_max, ep.deck_full, (1u << C) - 1u, (1u << R) - 1u, C * R,
                 C * R + C + R, R == 1 ? 3 : 2 * R};
  }
};

// ---- mt19937, incremental form -----------------------------------------------------------------
// The generator state is advanced one word per draw:  x[i] <- x[i+397] ^ twist(x[i], x[i+1]),
// output = temper(x[i]) — identical to std::mt19937's batch regeneration, without the 624-word stall.
constexpr uint32_t kMtUpper = 0x80000000u, kMtLower = 0x7fffffffu, kMtMag = 0x9908b0dfu;

__device__ __forceinline__ uint32_t mt_temper(uint32_t x) {
  x ^= x >> 11;
  x ^= (x << 7) & 0x9d2c5680u;
  x ^= (x << 15) & 0xefc60000u;
  x ^= x >> 18;
  return x;
}
__device__ __forceinline__ uint32_t mt_twist(uint32_t xi, uint32_t xi1, uint32_t xim) {
  const uint32_t y = (xi & kMtUpper) | (xi1 & kMtLower);
  return xim ^ (y >> 1) ^ ((y & 1u) ? kMtMag : 0u);
}
__device__ __forceinline__ uint32_t wrap624(uint32_t i) { return i >= (uint32_t)kMtN ? i - kMtN : i; }

// Per-lane RNG context for one kernel invocation.  Draws are served, in order, from
//  (1) the two look-ahead outputs carried in the state planes (regenerated off the critical path),
//  (2) the reset kernel's LDS prefetch window (new state words for positions wbase+k, not yet in HBM),
//  (3) the memory slow path (three dependent loads + one store per draw).
struct Rng {
  uint32_t* mt;
  uint32_t draws;  // logical draws consumed
  uint32_t la0, la1;
  int la_n;
  uint32_t spos;  // memory position the slow path regenerates next
  uint32_t* win;  // LDS, lane-strided by kWave; nullptr when there is no window
  int w_c, w_n;
};

__device__ __forceinline__ uint32_t rng_next(Rng& r) {
  r.draws += 1;
  if (r.la_n > 0) {
    const uint32_t v = r.la0;
    r.la0 = r.la1;
    r.la_n -= 1;
    return v;
  }
  if (r.w_c < r.w_n) {
    const uint32_t v = mt_temper(r.win[r.w_c * kWave]);
    r.w_c += 1;
    return v;
  }
  const uint32_t i = r.spos;
  const uint32_t x = mt_twist(r.mt[i], r.mt[wrap624(i + 1)], r.mt[wrap624(i + kMtM)]);
  r.mt[i] = x;
  r.spos = wrap624(i + 1);
  return mt_temper(x);
}

__device__ __forceinline__ void la_push(Rng& r, uint32_t out) {
  if (r.la_n == 0)
    r.la0 = out;
  else
    r.la1 = out;
  r.la_n += 1;
}

// Look-ahead refill, split so the loads are in flight while the observation rows are built.
struct Refill {
  uint32_t pos, r0, r1, r2, m0, m1;
  int need;
};
__device__ __forceinline__ void refill_issue(Refill& f, const Rng& r, bool active) {
  f.need = active ? 2 - r.la_n : 0;
  f.pos = r.spos;
  f.r0 = f.r1 = f.r2 = f.m0 = f.m1 = 0;
  if (f.need > 0) {
    const uint32_t i = f.pos;
    f.r0 = r.mt[i];
    f.r1 = r.mt[wrap624(i + 1)];
    f.r2 = r.mt[wrap624(i + 2)];
    f.m0 = r.mt[wrap624(i + kMtM)];
    f.m1 = r.mt[wrap624(i + 1 + kMtM)];
  }
}
__device__ __forceinline__ void refill_finish(const Refill& f, Rng& r) {
  if (f.need > 0) {
    const uint32_t x0 = mt_twist(f.r0, f.r1, f.m0);
    r.mt[f.pos] = x0;
    la_push(r, mt_temper(x0));
    r.spos = wrap624(f.pos + 1);
    if (f.need > 1) {
      const uint32_t x1 = mt_twist(f.r1, f.r2, f.m1);
      r.mt[r.spos] = x1;
      la_push(r, mt_temper(x1));
      r.spos = wrap624(r.spos + 1);
    }
  }
}

// libstdc++ uniform_int_distribution<>::_S_nd (Lemire) on a 32-bit generator: value in [0, range)
__device__ __forceinline__ uint32_t uniform_below(uint32_t range, Rng& r) {
  uint64_t product = (uint64_t)rng_next(r) * (uint64_t)range;
  uint32_t low = (uint32_t)product;
  if (low < range) {
    const uint32_t threshold = (0u - range) % range;
    while (low < threshold) {
      product = (uint64_t)rng_next(r) * (uint64_t)range;
      low = (uint32_t)product;
    }
  }
  return (uint32_t)(product >> 32);
}

// Literal restatement of std::discrete_distribution<>(probs)(rng) with probs = count/deck_size
// (libstdc++ random.tcc: normalise by the sequential sum, partial sums, last := 1.0,
// p = generate_canonical<double,53> = (u1 + u2*2^32)/2^64, index = lower_bound(cp, p)).
__device__ __noinline__ int deal_pick_exact(uint64_t deck, int deck_size, uint32_t u1, uint32_t u2) {
  int last_t = -1;
#pragma unroll
  for (int t = 0; t < 25; ++t)
    if (cnt2(deck, t)) last_t = t;
  const double D = (double)deck_size;
  const double w1 = 1.0 / D, w2 = 2.0 / D, w3 = 3.0 / D;
  double sum = 0.0;
#pragma unroll
  for (int t = 0; t < 25; ++t) {
    const uint32_t c = cnt2(deck, t);
    if (c) sum += (c == 1 ? w1 : (c == 2 ? w2 : w3));
  }
  const double p1 = w1 / sum, p2 = w2 / sum, p3 = w3 / sum;
  double u = ((double)u1 + (double)u2 * 4294967296.0) / 18446744073709551616.0;
  if (u >= 1.0) u = 0x1.fffffffffffffp-1;  // nextafter(1, 0)
  double cum = 0.0;
  int pick = -1;
#pragma unroll
  for (int t = 0; t < 25; ++t) {
    const uint32_t c = cnt2(deck, t);
    if (c) {
      cum += (c == 1 ? p1 : (c == 2 ? p2 : p3));
      const double cp = (t == last_t) ? 1.0 : cum;
      if (pick < 0 && cp >= u) pick = t;
    }
  }
  return pick;
}

// HanabiState::ApplyRandomChance: returns the dealt card type.  Consumes two draws unless fewer than
// two card types remain (libstdc++ then returns index 0 without touching the generator).
//
// Fast path (deal_mode 0): in exact arithmetic the pick is the first type whose cumulative count C_t
// satisfies C_t/D >= S/2^64 with S = u1 + u2*2^32.  The fp64 computation above perturbs each side by
// < 2^-47 (<= 55 roundings of 2^-53 on values <= 1), i.e. by < 2^-41.3 after scaling by D <= 50, so
// whenever frac(S*D/2^64) lies in [2^-36, 1-2^-36] both give the same index; otherwise (probability
// 2^-35 per deal) the literal fp64 restatement decides.  deal_mode 1 forces the literal path.
__device__ __forceinline__ int deal_pick(int deal_mode, uint64_t deck, int deck_size, Rng& r) {
  const uint64_t nz = (deck | (deck >> 1)) & 0x5555555555555555ull;
  if (__popcll(nz) < 2) return (int)(__builtin_ctzll(nz) >> 1);
  const uint32_t u1 = rng_next(r);
  const uint32_t u2 = rng_next(r);
  if (deal_mode == 0) {
    const uint64_t S = (uint64_t)u1 | ((uint64_t)u2 << 32);
    const uint64_t lo = S * (uint64_t)deck_size;
    const uint64_t hi = __umul64hi(S, (uint64_t)deck_size);
    if (lo >= (1ull << 28) && lo <= 0ull - (1ull << 28)) {
      return df_pick(deck, (uint32_t)hi + 1u);   // hi < deck_size: 1 <= need <= cards in the deck
    }
  }
  return deal_pick_exact(deck, deck_size, u1, u2);
}

// ---- small packed-field helpers -----------------------------------------------------------------
__device__ __forceinline__ uint32_t remove_field(uint32_t x, int i, int w, int nfields) {
  const uint32_t total_mask = (nfields * w >= 32) ? 0xffffffffu : ((1u << (nfields * w)) - 1u);
  const uint32_t body = x & total_mask;
  const uint32_t low = body & ((1u << (i * w)) - 1u);
  const uint32_t high = ((i + 1) * w >= 32) ? 0u : (body >> ((i + 1) * w));
  return (x & ~total_mask) | low | (high << (i * w));
}

struct MoveDec {
  int type;  // 0 invalid, 1 play, 2 discard, 3 reveal colour, 4 reveal rank
  int idx;   // card index
  int off;   // target offset
  int val;   // colour or rank
};

// HanabiGame::GetMove: uid order discard, play, reveal colour, reveal rank
__device__ __forceinline__ MoveDec decode_uid(int uid, int P, int H) {
  MoveDec m{0, 0, 0, 0};
  if (uid < 0) return m;
  if (uid < H) {
    m.type = 2;
    m.idx = uid;
    return m;
  }
  uid -= H;
  if (uid < H) {
    m.type = 1;
    m.idx = uid;
    return m;
  }
  uid -= H;
  if (uid < (P - 1) * 5) {
    m.type = 3;
    m.off = 1 + uid / 5;
    m.val = uid % 5;
    return m;
  }
  uid -= (P - 1) * 5;
  if (uid < (P - 1) * 5) {
    m.type = 4;
    m.off = 1 + uid / 5;
    m.val = uid % 5;
    return m;
  }
  return m;
}

// the same for a variant's C colours and R ranks
__device__ __forceinline__ MoveDec decode_uid(int uid, int P, int H, const Rules& ru) {
  MoveDec m{0, 0, 0, 0};
  if (uid < 0) return m;
  if (uid < H) {
    m.type = 2;
    m.idx = uid;
    return m;
  }
  uid -= H;
  if (uid < H) {
    m.type = 1;
    m.idx = uid;
    return m;
  }
  uid -= H;
  if (uid < (P - 1) * ru.C) {
    m.type = 3;
    m.off = 1 + uid / ru.C;
    m.val = uid % ru.C;
    return m;
  }
  uid -= (P - 1) * ru.C;
  if (uid < (P - 1) * ru.R) {
    m.type = 4;
    m.off = 1 + uid / ru.R;
    m.val = uid % ru.R;
    return m;
  }
  return m;
}

__device__ __forceinline__ MoveDec decode_uid(int uid, int P, int H, const FullRules&) { return decode_uid(uid, P, H); }

// per-slot match mask of a packed hand word; cards are 5-bit colour*5+rank
__device__ __forceinline__ uint32_t hand_match_mask(uint32_t hw, bool by_color, int val) {
  const int len = (hw >> 25) & 7;
  uint32_t m = 0;
#pragma unroll
  for (int i = 0; i < 5; ++i) {
    const int card = (hw >> (5 * i)) & 31;
    const int c = (card * 13) >> 6;  // card / 5 for card < 32
    const int r = card - 5 * c;
    if (i < len && (by_color ? c : r) == val) m |= 1u << i;
  }
  return m;
}

#define ST(pl) s_st[(pl) * kWave + lane]
// Stamp slots.  Legacy layout [grid][8] (dbg_iters = 0): slots 0-7 of the one record of the launch.  Trace layout
// [grid][dbg_iters][16] (dbg_iters > 0): one record per iteration `it` of a persistent launch (iterations past dbg_iters share the last).
//   env_body (single-phase):   0 iteration start, 1 planes staged in LDS (wave 0's first waited load + barrier), 2 logic done (barrier),
//                              3 rows built, 4 planes written back (barrier), 5 rows streamed (thread 0), 6 / 7 reset: window loaded / dealt
//   env_rollout_pipe_kernel:   0 iteration start, 1 wave 0's outstanding stores drained (s_waitcnt vmcnt(0), trace layout only),
//                              11 wave 0's logic done, 2 end of phase A (barrier), 3 rows built, 4 end of phase B (barrier),
//                              8 stream wave (thread 64): rows of `it - 1` streamed and cleared, 5 last record only: epilogue stream done,
//                              6 / 7 as above
//                              12 pacing: ticks by which the stream of this iteration's rows is delayed (pace_delay)
//                              13 delta stream (EnvParams::delta): 128-byte lines of priv_s the stream wave stored for the rows of `it - 1`
//                                 (with half-line units: lines with any change); the units themselves go to EnvParams::dbg_units_lo / _hi
//                              14 / 15 last record only: lines wave 0 / wave 1 stored in the epilogue stream
//   both, trace layout:        9 HW_REG_HW_ID, 10 HW_REG_XCC_ID of the workgroup (written with slot 0); env_rollout_pipe_kernel: 9 is
//                              the logic wave's, and the upper 32 bits of 10 hold the stream wave's HW_REG_HW_ID
__device__ __forceinline__ void env_stamp(const EnvParams& ep, int it, int k, unsigned long long v) {
  const size_t blk = (size_t)(ep.g_begin / ep.gpw) + blockIdx.x;
  if (ep.dbg_iters > 0)
    ep.dbg[(blk * ep.dbg_iters + (size_t)min(it, ep.dbg_iters - 1)) * 16 + k] = v;
  else if (k < 8)
    ep.dbg[((size_t)(ep.g_begin / kWave) + blockIdx.x) * 8 + k] = v;
}
#define STAMP_T(k, t)                                                                                   \
  do {                                                                                                  \
    if (ep.dbg && threadIdx.x == (t)) env_stamp(ep, dbg_it, (k), wall_clock64());                      \
  } while (0)
#define STAMP(k) STAMP_T(k, 0)
// slot 0 of an iteration, plus (trace layout) where the workgroup runs
#define STAMP_START()                                                                                   \
  do {                                                                                                  \
    if (ep.dbg && threadIdx.x == 0) {                                                                   \
      env_stamp(ep, dbg_it, 0, wall_clock64());                                                         \
      if (ep.dbg_iters > 0) {                                                                           \
        unsigned hw_id, xcc_id;                                                                         \
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw_id));                            \
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc_id));                          \
        env_stamp(ep, dbg_it, 9, hw_id);                                                                \
        env_stamp(ep, dbg_it, 10, xcc_id);                                                              \
      }                                                                                                 \
    }                                                                                                   \
  } while (0)
// env_rollout_pipe_kernel's form: slot 10 also carries the stream wave's HW_REG_HW_ID (`stream_hw`, an LDS word that wave wrote
// in the prologue) in its upper 32 bits; the XCC id stays in bits 0-3
#define STAMP_START_PIPE(stream_hw)                                                                     \
  do {                                                                                                  \
    if (ep.dbg && threadIdx.x == 0) {                                                                   \
      env_stamp(ep, dbg_it, 0, wall_clock64());                                                         \
      if (ep.dbg_iters > 0) {                                                                           \
        unsigned hw_id, xcc_id;                                                                         \
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw_id));                            \
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc_id));                          \
        env_stamp(ep, dbg_it, 9, hw_id);                                                                \
        env_stamp(ep, dbg_it, 10, ((unsigned long long)(stream_hw) << 32) | xcc_id);                    \
      }                                                                                                 \
    }                                                                                                   \
  } while (0)

// ---- the planes of a wave's 64 games between global memory and LDS, and the generator context that lives in them ---------------
// Used by the playout body and env_observe_kernel.  NOT by env_body and env_rollout_pipe_kernel, which spell the same sequences out:
// calling these helpers there changes the register allocation and instruction order of every env_kernel, scripted-step and rollout
// instance (measured when the helpers were introduced, tools/isa_compare.py: env_rollout_pipe_kernel<2,5> 213 -> 212 VGPRs and
// 436 bytes shorter, <4,4> 1,276 bytes longer), and those kernels are what bench.py times.  Leave them spelled out.
//
// all npl planes of game g -> s_st (loads issued in batches of 8 so they overlap)
__device__ __forceinline__ void stage_planes(const EnvParams& ep, uint32_t* s_st, int lane, int g) {
  for (int pl0 = 0; pl0 < ep.npl; pl0 += 8) {
    uint32_t v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = ep.planes[(size_t)min(pl0 + j, ep.npl - 1) * ep.Gpad + g];
#pragma unroll
    for (int j = 0; j < 8; ++j)
      if (pl0 + j < ep.npl) ST(pl0 + j) = v[j];
  }
}
// game g's generator as the staged planes describe it (no prefetch window); misc: the game's PL_MISC word, which every caller holds
__device__ __forceinline__ Rng rng_open(const EnvParams& ep, const uint32_t* s_st, int lane, int g, uint32_t misc) {
  Rng rng;
  rng.mt = ep.mt + (size_t)g * kMtN;
  rng.draws = ST(PL_DRAWS);
  rng.la0 = ST(PL_LA0);
  rng.la1 = ST(PL_LA1);
  rng.la_n = misc_la_n(misc);
  rng.spos = (rng.draws + (uint32_t)rng.la_n) % (uint32_t)kMtN;
  rng.win = nullptr;
  rng.w_c = rng.w_n = 0;
  return rng;
}
// ... and back into the staged planes
__device__ __forceinline__ void rng_close(const Rng& rng, uint32_t* s_st, int lane) {
  ST(PL_DRAWS) = rng.draws;
  ST(PL_LA0) = rng.la0;
  ST(PL_LA1) = rng.la1;
  ST(PL_MISC) = (ST(PL_MISC) & ~(3u << 22)) | ((uint32_t)rng.la_n << 22);
}

template <class Ru>
__device__ __forceinline__ bool move_is_legal(int P, const uint32_t* s_st, int lane, const MoveDec& m, const Ru& ru) {
  const uint32_t board = ST(PL_BOARD);
  const int cur = board_cur(board);
  if (m.type == 0 || cur < 0) return false;
  if (m.type == 1 || m.type == 2) {
    if (m.type == 2 && board_info(board) >= ru.MI) return false;
    const int len = (ST(PLH(cur)) >> 25) & 7;
    return m.idx < len;
  }
  if (board_info(board) <= 0) return false;
  if (m.off < 1 || m.off >= P) return false;
  int q = cur + m.off;
  if (q >= P) q -= P;
  return hand_match_mask(ST(PLH(q)), m.type == 3, m.val) != 0;
}

// history-item record of `move` applied by the player on turn in the current state (no mutation);
// also used for the SAD greedy move (the reference applies it to a clone only to read this back:
// cpp/hanabi_env.cc:82-91).
template <class Ru>
__device__ __forceinline__ uint32_t make_history(int P, const uint32_t* s_st, int lane, const MoveDec& m, const Ru& ru) {
  const uint32_t board = ST(PL_BOARD);
  const int cur = board_cur(board);
  uint32_t rec = (uint32_t)m.type | ((uint32_t)cur << 3);
  if (m.type == 1 || m.type == 2) {
    const uint32_t hw = ST(PLH(cur));
    const int card = (hw >> (5 * m.idx)) & 31;
    const int c = (card * 13) >> 6, r = card - 5 * c;
    rec |= (uint32_t)m.idx << 15;
    rec |= (uint32_t)c << 23;
    rec |= (uint32_t)r << 26;
    if (m.type == 2) {
      if (board_info(board) < ru.MI) rec |= 1u << 30;
    } else {
      if (r == board_fw(board, c)) {
        rec |= 1u << 29;
        if (r + 1 == ru.R && board_info(board) < ru.MI) rec |= 1u << 30;
      }
    }
  } else {
    int q = cur + m.off;
    if (q >= P) q -= P;
    rec |= (uint32_t)m.off << 6;
    rec |= (uint32_t)m.val << (m.type == 3 ? 9 : 12);
    rec |= hand_match_mask(ST(PLH(q)), m.type == 3, m.val) << 18;
  }
  return rec;
}

// HanabiState::AdvanceToNextPlayer
__device__ __forceinline__ uint32_t advance_player(int P, int H, const uint32_t* s_st, int lane, uint32_t board,
                                                   int deck_size) {
  bool short_hand = false;
  for (int p = 0; p < P; ++p) short_hand |= (int)((ST(PLH(p)) >> 25) & 7) < H;
  if (deck_size > 0 && short_hand) {
    board = board_set(board, 24, 7u, 0u);  // chance player (-1)
  } else {
    const int nxt = board_next(board);
    board = board_set(board, 24, 7u, (uint32_t)(nxt + 1));
    int nn = nxt + 1;
    if (nn >= P) nn = 0;
    board = board_set(board, 27, 7u, (uint32_t)nn);
  }
  return board;
}

// the next card type to deal.  ScriptedParams (the scripted step only): while the deal index is below the game's script length the
// card is the script's and no generator draw is consumed; a scripted card the deck does not hold (a game forked over a script that
// was validated for another) is logged as code 5 and dealt from the generator instead
__device__ __forceinline__ void log_error(const EnvParams& ep, int g, int code);   // defined with the error log below
template <class EP, class Ru>
__device__ __forceinline__ int next_card(const EP& ep, uint64_t deck, int deck_size, Rng& rng, int g, const Ru& ru) {
  if constexpr (EP::kScripted) {
    const int di = ru.deck - deck_size;
    if (di < ep.sc.count[g]) {
      const int t = (int)ep.sc.cards[(size_t)g * 52 + di];
      if (t < 25 && cnt2(deck, t) != 0u) return t;
      log_error(ep, g, 5);
    }
  }
  return deal_pick(ep.deal_mode, deck, deck_size, rng);
}

// deal one card to the first short hand (kDeal branch of HanabiState::ApplyMove + ApplyRandomChance)
template <class EP, class Ru>
__device__ __forceinline__ void deal_one(const EP& ep, int P, int H, uint32_t* s_st, int lane, Rng& rng,
                                         int g, const Ru& ru) {
  uint64_t deck = (uint64_t)ST(PL_DECK_LO) | ((uint64_t)ST(PL_DECK_HI) << 32);
  uint32_t misc = ST(PL_MISC);
  int deck_size = (misc >> 8) & 63;
  const int t = next_card(ep, deck, deck_size, rng, g, ru);
  deck -= (uint64_t)1 << (2 * t);
  ST(PL_DECK_LO) = (uint32_t)deck;
  ST(PL_DECK_HI) = (uint32_t)(deck >> 32);
  if (ep.track_dh) ep.deck_hist[(size_t)g * 52 + (ru.deck - deck_size)] = (uint8_t)t;
  deck_size -= 1;
  misc = (misc & ~(63u << 8)) | ((uint32_t)deck_size << 8);
  ST(PL_MISC) = misc;
  int to = 0;
  for (int p = P - 1; p >= 0; --p)
    if ((int)((ST(PLH(p)) >> 25) & 7) < H) to = p;
  uint32_t hw = ST(PLH(to));
  const int len = (hw >> 25) & 7;
  hw = (hw & ~(7u << 25)) | ((uint32_t)t << (5 * len)) | ((uint32_t)(len + 1) << 25);
  ST(PLH(to)) = hw;
  ST(PLKCP(to)) |= ru.cmask << (5 * len);
  ST(PLKRP(to)) |= ru.rmask << (5 * len);
  ST(PLKH(to)) &= ~(63u << (6 * len));
  ST(PL_BOARD) = advance_player(P, H, s_st, lane, ST(PL_BOARD), deck_size);
}

// ---- LDS bit-row helpers (branch-free: OR-ing zero is a no-op) ------------------------------------
__device__ __forceinline__ void or_bit(uint32_t* b, uint32_t pos) { atomicOr(&b[pos >> 5], 1u << (pos & 31)); }
__device__ __forceinline__ void or_bits32(uint32_t* b, uint32_t pos, uint32_t val) {
  const uint32_t w = pos >> 5, s = pos & 31;
  const uint64_t v = (uint64_t)val << s;
  atomicOr(&b[w], (uint32_t)v);
  atomicOr(&b[w + 1], (uint32_t)(v >> 32));
}
__device__ __forceinline__ void or_bits64(uint32_t* b, uint32_t pos, uint64_t val) {
  const uint32_t w = pos >> 5, s = pos & 31;
  const uint64_t lo = val << s;
  atomicOr(&b[w], (uint32_t)lo);
  atomicOr(&b[w + 1], (uint32_t)(lo >> 32));
  atomicOr(&b[w + 2], ((uint32_t)(val >> 32) >> (31u - s)) >> 1);
}

__device__ __forceinline__ uint32_t get4(const uint32_t* bits, uint32_t bp) {
  const uint32_t w = bp >> 5, s = bp & 31;
  const uint32_t lo = bits[w];
  if (s <= 28) return (lo >> s) & 15u;
  const uint32_t hi = bits[w + 1];
  return ((lo >> s) | (hi << (32 - s))) & 15u;
}
__device__ __forceinline__ uint32_t get1(const uint32_t* bits, uint32_t bp) { return (bits[bp >> 5] >> (bp & 31)) & 1u; }

__device__ __forceinline__ float4 nib_to_f4(uint32_t nib) {
  float4 v;
  v.x = (nib & 1u) ? 1.f : 0.f;
  v.y = (nib & 2u) ? 1.f : 0.f;
  v.z = (nib & 4u) ? 1.f : 0.f;
  v.w = (nib & 8u) ? 1.f : 0.f;
  return v;
}

// 64 bits from an arbitrary bit position of an LDS bit array (may read up to two words past the last one it needs: callers
// mask, and the arrays are followed by other LDS data of the same workgroup)
__device__ __forceinline__ uint64_t get64(const uint32_t* bits, uint32_t bp) {
  const uint32_t w = bp >> 5, s = bp & 31;
  uint64_t v = ((uint64_t)bits[w] | ((uint64_t)bits[w + 1] << 32)) >> s;
  if (s) v |= (uint64_t)bits[w + 2] << (64u - s);
  return v;
}
__device__ __forceinline__ uint32_t get8(const uint32_t* bits, uint32_t bp) {
  const uint32_t w = bp >> 5, s = bp & 31;
  const uint32_t lo = bits[w];
  if (s <= 24) return (lo >> s) & 255u;
  return ((lo >> s) | (bits[w + 1] << (32 - s))) & 255u;
}

// rows [row0, row0 + nrows) of the workgroup's LDS observation bit rows (row r = bits r*F .. r*F+F-1) as
//   bit words   priv_bits[(grow0 + r) * pw64 + k]          (the replay's HSAD_BITS format: LSB first, tail bits zero)
//   bf16 rows   priv16[(grow0 + r) * ld16 + j]             (1.0 = 0x3F80; columns >= F zero)
__device__ __forceinline__ void stream_rows_packed(const EnvParams& ep, const uint32_t* s_obs, int row0, int nrows, size_t grow0,
                                                   int tid, int nthreads) {
  const uint32_t F = (uint32_t)ep.F;
  if (ep.priv_bits) {
    const int pw = ep.pw64;
    for (int k = tid; k < nrows * pw; k += nthreads) {
      const int r = k / pw, wd = k - r * pw;
      const uint32_t left = F - (uint32_t)wd * 64u;
      uint64_t v = get64(s_obs, (uint32_t)(row0 + r) * F + (uint32_t)wd * 64u);
      if (left < 64u) v &= (1ull << left) - 1ull;
      ep.priv_bits[(grow0 + r) * pw + wd] = v;
    }
  }
  if (ep.priv16) {
    const int cpr = ep.ld16 >> 3;  // 16-byte chunks (8 values) per row
    for (int k = tid; k < nrows * cpr; k += nthreads) {
      const int r = k / cpr, c = k - r * cpr;
      const uint32_t j0 = (uint32_t)c * 8u;
      uint32_t m = 0;
      if (j0 < F) {
        m = get8(s_obs, (uint32_t)(row0 + r) * F + j0);
        if (F - j0 < 8u) m &= (1u << (F - j0)) - 1u;
      }
      uint4 o;
      o.x = ((m & 1u) ? 0x3F80u : 0u) | ((m & 2u) ? 0x3F800000u : 0u);
      o.y = ((m & 4u) ? 0x3F80u : 0u) | ((m & 8u) ? 0x3F800000u : 0u);
      o.z = ((m & 16u) ? 0x3F80u : 0u) | ((m & 32u) ? 0x3F800000u : 0u);
      o.w = ((m & 64u) ? 0x3F80u : 0u) | ((m & 128u) ? 0x3F800000u : 0u);
      *reinterpret_cast<uint4*>(ep.priv16 + (grow0 + r) * (size_t)ep.ld16 + j0) = o;
    }
  }
}

// out[i] = bit(bit0 + i) ? 1.f : 0.f for i in [0, n): 16-byte stores wherever the address allows.
__device__ __forceinline__ void stream_bits_f32(const uint32_t* bits, uint32_t bit0, float* out, uint32_t n, int lane) {
  const uintptr_t addr = (uintptr_t)out;
  uint32_t head = (uint32_t)(((16u - (uint32_t)(addr & 15u)) & 15u) >> 2);
  if (head > n) head = n;
  if ((uint32_t)lane < head) out[lane] = get1(bits, bit0 + lane) ? 1.f : 0.f;
  const uint32_t nbody = (n - head) >> 2;
  float4* o4 = reinterpret_cast<float4*>(out + head);
  const uint32_t b1 = bit0 + head;
  for (uint32_t k = lane; k < nbody; k += kWave) o4[k] = nib_to_f4(get4(bits, b1 + 4u * k));
  const uint32_t done = head + 4u * nbody;
  if ((uint32_t)lane < n - done) out[done + lane] = get1(bits, bit0 + done + lane) ? 1.f : 0.f;
}

// Same, for the wave-wide aligned case (bit0 == 0, out 16-byte aligned): every lane reads one 32-bit word
// of bits and emits 8 consecutive float4 — 128 B per lane per iteration, 8 KiB per wave-iteration.
template <bool NT>
__device__ __forceinline__ void stream_bits_f32_aligned(const uint32_t* bits, float* out, uint32_t n, int lane,
                                                        int nthreads = kWave) {
  float4* o4 = reinterpret_cast<float4*>(out);
  const uint32_t nch = n >> 2;
  for (uint32_t k = lane; k < nch; k += nthreads) {
    const float4 v = nib_to_f4((bits[k >> 3] >> ((k & 7u) * 4u)) & 15u);
    if (NT) {
      typedef float nt_f4 __attribute__((ext_vector_type(4)));
      nt_f4 w = {v.x, v.y, v.z, v.w};
      __builtin_nontemporal_store(w, reinterpret_cast<nt_f4*>(o4 + k));
    } else {
      o4[k] = v;
    }
  }
  const uint32_t done = nch << 2;
  if ((uint32_t)lane < n - done) out[done + lane] = get1(bits, done + lane) ? 1.f : 0.f;
}

// Same, but only where the bits changed: `old` holds the bit words this range of `out` was last written from.  Word w is the eight
// float4 of chunks 8w .. 8w+7, one 128-byte line of `out` (the range starts on a line), so a line is stored iff its word differs and
// no line is ever stored in part.  all: every line regardless (`old` is not read).  The tail floats (n & 3) are always stored.
// Returns this lane's count of stored lines (count on).
template <bool NT>
__device__ __forceinline__ unsigned stream_bits_f32_delta(const uint32_t* bits, const uint32_t* old, bool all, float* out, uint32_t n,
                                                          int lane, int nthreads, bool count) {
  float4* o4 = reinterpret_cast<float4*>(out);
  const uint32_t nch = n >> 2;
  unsigned stored = 0;
  for (uint32_t k = lane; k < nch; k += nthreads) {
    const uint32_t w = bits[k >> 3];
    if (all || w != old[k >> 3]) {
      const float4 v = nib_to_f4((w >> ((k & 7u) * 4u)) & 15u);
      if (NT) {
        typedef float nt_f4 __attribute__((ext_vector_type(4)));
        nt_f4 q = {v.x, v.y, v.z, v.w};
        __builtin_nontemporal_store(q, reinterpret_cast<nt_f4*>(o4 + k));
      } else {
        o4[k] = v;
      }
      if (count && (k & 7u) == 0u) ++stored;
    }
  }
  const uint32_t done = nch << 2;
  if ((uint32_t)lane < n - done) out[done + lane] = get1(bits, done + lane) ? 1.f : 0.f;
  return stored;
}

// The compacted form of the same (EnvParams::compact), for one wave and a stream that is not an `all` stream: first a scan that
// lists the changed units, then a store loop over the list only, whole units per wave-store, without a predicate and with
// several groups of LDS reads in flight.  UNIT is the floats of a unit: 32 (a word of bits, one 128-byte line: stores exactly the
// lines the direct form stores) or 16 (a half word, one 64-byte half line, which is one native request of the L2 to the memory
// fabric: a line whose change sits in one half costs half the bytes).  Returns the number of 128-byte lines with any change in
// lane 0 and 0 in every other lane (the direct form's per-lane counts sum to the same); units: the units stored, likewise.
//
// The list costs no LDS: entry r is written in place to position r of list, which is `old` itself.
//   UNIT 32: entries are word indices, 32 bits wide.  Invariant: scan step s reads positions [64s, 64s + 64) and lane l's entry
//   goes to position base_s + rank <= 64s + l, base_s being the number of changed words before step s and rank the number of
//   changed lanes below l.  So a write of step s lands only on a position that step s or an earlier one has read, and every later
//   step reads only positions >= 64(s + 1): no read of `old` ever sees a list entry.
//   UNIT 16: entries are half-line indices 2w and 2w + 1, 16 bits wide (the largest is 2 x 14,390 for five players with SAD in
//   64-game workgroups), entry r at half-word r.  Scan step s reads words [64s, 64s + 64), that is half-words [128s, 128s + 128).
//   At most 128s entries exist before step s and lane l's one or two entries (hi directly after lo, so that the halves of a line
//   are neighbours in the list and their stores still form one 128-byte segment) go to half-words <= 128s + 2l + 1: inside the
//   word that lane itself read in this step, or below.  Again no read of `old` ever sees an entry.
// Within a step the compare -> ballot -> rank dependence puts the step's reads before its writes.  The scan below takes kScanSteps
// steps' reads together ahead of their writes, which keeps the invariant: those writes land below word 64(s + kScanSteps) at most,
// all read by then.  A partial last word (n / 4 not a multiple of 8) is not listed: its position is beyond every entry, and the
// lanes of its chunks store it whole in the direct form, whichever the unit.  The caller clears `old`, list included, afterwards.
constexpr int kScanSteps = 4;    // scan steps whose LDS reads are issued together
constexpr int kStoreGroups = 4;  // store groups (1 KiB each: eight lines or sixteen halves) whose LDS reads are issued together

template <bool NT>
__device__ __forceinline__ void store_chunk(float4* p, const float4 v) {
  if (NT) {
    typedef float nt_f4 __attribute__((ext_vector_type(4)));
    nt_f4 q = {v.x, v.y, v.z, v.w};
    __builtin_nontemporal_store(q, reinterpret_cast<nt_f4*>(p));
  } else {
    *p = v;
  }
}

typedef uint16_t __attribute__((may_alias)) list16_t;   // the half-line list lives in the words of `old`

template <bool NT, int UNIT>
__device__ __forceinline__ unsigned stream_bits_f32_compact(const uint32_t* bits, uint32_t* list, float* out, uint32_t n, int lane,
                                                            unsigned& units) {
  static_assert(UNIT == 32 || UNIT == 16, "a unit is a line or a half line");
  float4* o4 = reinterpret_cast<float4*>(out);
  list16_t* list16 = reinterpret_cast<list16_t*>(list);
  const uint32_t nch = n >> 2;
  const uint32_t nfull = nch >> 3;   // words that own eight chunks
  // scan: count (entries) and lines are wave-uniform
  uint32_t count = 0, lines = 0;
  for (uint32_t w0 = 0; w0 < nfull; w0 += 64u * kScanSteps) {
    uint32_t b[kScanSteps], o[kScanSteps];
#pragma unroll
    for (int u = 0; u < kScanSteps; ++u) {
      const uint32_t w = min(w0 + 64u * u + (uint32_t)lane, nfull - 1u);
      b[u] = bits[w];
      o[u] = list[w];
    }
#pragma unroll
    for (int u = 0; u < kScanSteps; ++u) {
      const uint32_t w = w0 + 64u * u + (uint32_t)lane;
      if (UNIT == 32) {
        const bool changed = w < nfull && b[u] != o[u];
        const unsigned long long m = __ballot(changed);
        const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
        if (changed) list[count + rank] = w;
        count += (uint32_t)__popcll(m);
      } else {
        const uint32_t x = w < nfull ? b[u] ^ o[u] : 0u;
        const bool lo = (x & 0xffffu) != 0u, hi = (x >> 16) != 0u;
        const unsigned long long m_lo = __ballot(lo), m_hi = __ballot(hi);
        uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(m_lo >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m_lo, 0u));
        rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(m_hi >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m_hi, rank));
        if (lo) list16[count + rank] = (list16_t)(2u * w);
        if (hi) list16[count + rank + (lo ? 1u : 0u)] = (list16_t)(2u * w + 1u);
        count += (uint32_t)__popcll(m_lo) + (uint32_t)__popcll(m_hi);
        lines += (uint32_t)__popcll(m_lo | m_hi);
      }
    }
  }
  if (UNIT == 32) lines = count;
  // the partial last word, read before anything else is done (no entry reaches its position)
  const uint32_t kp = 8u * nfull + (uint32_t)lane;
  const bool part = kp < nch;   // lanes 0 .. (nch & 7) - 1
  uint32_t wp = 0u;
  bool part_changed = false;
  if (part) {
    wp = bits[nfull];
    part_changed = wp != list[nfull];
  }
  if (UNIT == 32) {
    // store: lane l serves entry 8j + (l >> 3) of group j, chunk l & 7 of its line
    const uint32_t sub = (uint32_t)lane >> 3, c = (uint32_t)lane & 7u;
    uint32_t e0 = 0;
    for (; e0 + 8u * kStoreGroups <= count; e0 += 8u * kStoreGroups) {
      uint32_t idx[kStoreGroups], word[kStoreGroups];
#pragma unroll
      for (int u = 0; u < kStoreGroups; ++u) idx[u] = list[e0 + 8u * u + sub];
#pragma unroll
      for (int u = 0; u < kStoreGroups; ++u) word[u] = bits[idx[u]];
#pragma unroll
      for (int u = 0; u < kStoreGroups; ++u) store_chunk<NT>(o4 + 8u * idx[u] + c, nib_to_f4((word[u] >> (4u * c)) & 15u));
    }
    if (e0 < count) {   // the last, partial block of groups: the lanes of entries >= count are off
      uint32_t idx[kStoreGroups], word[kStoreGroups];
#pragma unroll
      for (int u = 0; u < kStoreGroups; ++u) idx[u] = list[min(e0 + 8u * u + sub, count - 1u)];
#pragma unroll
      for (int u = 0; u < kStoreGroups; ++u) word[u] = bits[idx[u]];
#pragma unroll
      for (int u = 0; u < kStoreGroups; ++u)
        if (e0 + 8u * u + sub < count) store_chunk<NT>(o4 + 8u * idx[u] + c, nib_to_f4((word[u] >> (4u * c)) & 15u));
    }
  } else {
    // store: lane l serves entry 16j + (l >> 2) of group j, chunk l & 3 of its half line
    const uint32_t sub = (uint32_t)lane >> 2, c = (uint32_t)lane & 3u;
    uint32_t e0 = 0;
    for (; e0 + 16u * kStoreGroups <= count; e0 += 16u * kStoreGroups) {
      uint32_t idx[kStoreGroups], word[kStoreGroups];
#pragma unroll
      for (int u = 0; u < kStoreGroups; ++u) idx[u] = list16[e0 + 16u * u + sub];
#pragma unroll
      for (int u = 0; u < kStoreGroups; ++u) word[u] = bits[idx[u] >> 1];
#pragma unroll
      for (int u = 0; u < kStoreGroups; ++u)
        store_chunk<NT>(o4 + 4u * idx[u] + c, nib_to_f4((word[u] >> (16u * (idx[u] & 1u) + 4u * c)) & 15u));
    }
    if (e0 < count) {   // the last, partial block of groups: the lanes of entries >= count are off
      uint32_t idx[kStoreGroups], word[kStoreGroups];
#pragma unroll
      for (int u = 0; u < kStoreGroups; ++u) idx[u] = list16[min(e0 + 16u * u + sub, count - 1u)];
#pragma unroll
      for (int u = 0; u < kStoreGroups; ++u) word[u] = bits[idx[u] >> 1];
#pragma unroll
      for (int u = 0; u < kStoreGroups; ++u)
        if (e0 + 16u * u + sub < count)
          store_chunk<NT>(o4 + 4u * idx[u] + c, nib_to_f4((word[u] >> (16u * (idx[u] & 1u) + 4u * c)) & 15u));
    }
  }
  if (part_changed) store_chunk<NT>(o4 + kp, nib_to_f4((wp >> (4u * ((uint32_t)lane & 7u))) & 15u));
  const uint32_t done = nch << 2;
  if ((uint32_t)lane < n - done) out[done + lane] = get1(bits, done + lane) ? 1.f : 0.f;
  // the partial word went out whole: one line, and as many units as its chunks reach into
  const uint32_t part_units = UNIT == 32 || (nch & 7u) <= 4u ? 1u : 2u;
  units = lane == 0 ? count + (part_changed ? part_units : 0u) : 0u;
  return lane == 0 ? lines + (part_changed ? 1u : 0u) : 0u;
}

__device__ __forceinline__ uint32_t perm_c(uint32_t pm, int c) { return (pm >> (3 * c)) & 7u; }

template <class Ru>
__device__ __forceinline__ uint64_t encode_last_action(int P, int H, uint32_t rec, int observer, uint32_t pm, const Ru& ru) {
  const int type = rec & 7;
  if (!type) return 0;
  int rel = (int)((rec >> 3) & 7) - observer;
  if (rel < 0) rel += P;
  uint64_t m = 1ull << rel;
  int off = P;
  m |= 1ull << (off + type - 1);
  off += 4;
  if (type >= 3) {
    int tgt = rel + (int)((rec >> 6) & 7);
    if (tgt >= P) tgt -= P;
    m |= 1ull << (off + tgt);
  }
  off += P;
  if (type == 3) m |= 1ull << (off + perm_c(pm, (rec >> 9) & 7));
  off += ru.C;
  if (type == 4) m |= 1ull << (off + ((rec >> 12) & 7));
  off += ru.R;
  if (type >= 3) m |= (uint64_t)((rec >> 18) & 31u) << off;
  off += H;
  if (type <= 2) m |= 1ull << (off + ((rec >> 15) & 7));
  off += H;
  if (type <= 2) m |= 1ull << (off + perm_c(pm, (rec >> 23) & 7) * ru.R + ((rec >> 26) & 7));
  off += ru.CR;
  if (type == 1) m |= (uint64_t)((rec >> 29) & 3u) << off;
  return m;
}

// legal-move mask of player p in the current state (uids colour-permuted for that observer); noop iff nothing
// else is legal (HanabiState::LegalMoves + cpp/hanabi_env.cc:171-191)
template <int TH, class Ru>
__device__ __forceinline__ uint64_t legal_mask_of(int P, int H, int A, const uint32_t* s_st, int lane, int p, uint32_t pm,
                                                  const Ru& ru) {
  const uint32_t board = ST(PL_BOARD);
  const int cur = board_cur(board), info = board_info(board);
  uint64_t lm = 0;
  if (p == cur) {
    const uint32_t hw = ST(PLH(p));
    const int len = (hw >> 25) & 7;
    const uint64_t lenmask = (1ull << len) - 1ull;
    if (info < ru.MI) lm |= lenmask;
    lm |= lenmask << H;
    if (info > 0) {
      for (int o = 1; o < P; ++o) {
        int q = p + o;
        if (q >= P) q -= P;
        const uint32_t thw = ST(PLH(q));
        const int tl = (thw >> 25) & 7;
        uint32_t cm = 0, rm = 0;
#pragma unroll
        for (int i = 0; i < (TH ? TH : 5); ++i) {
          const int card = (thw >> (5 * i)) & 31;
          const int c = (card * 13) >> 6, r = card - 5 * c;
          if (i < tl) {
            cm |= 1u << perm_c(pm, c);
            rm |= 1u << r;
          }
        }
        lm |= (uint64_t)cm << (2 * H + (o - 1) * ru.C);
        lm |= (uint64_t)rm << (2 * H + (P - 1) * ru.C + (o - 1) * ru.R);
      }
    }
  }
  if (!lm) lm = 1ull << (A - 1);
  return lm;
}

// Build the observation / legal-move / own-hand bit rows of this lane's game for every observer
// (HanabiEnv::computeFeatureAndLegalMove, cpp/hanabi_env.cc:115-205, on top of the canonical encoder).
// FIXED (env_rollout_pipe_kernel, TP > 0, full rules): the observation row is assembled in registers at its compile-time bit positions
// and placed with one shifted write (hsad_obs_row.h) instead of field by field; the same bits.
template <int TP, int TH, bool V = false, bool FIXED = false>
__device__ __forceinline__ void build_rows(const EnvParams& ep, const uint32_t* s_st, int lane, int g, uint32_t* s_obs,
                                           uint32_t* s_legal, uint32_t* s_own, uint32_t greedy_rec, int p_begin,
                                           int p_step, uint32_t* s_lmask = nullptr) {
  const int P = TP ? TP : ep.P, H = TH ? TH : ep.H;
  const auto ru = RulesOf<V>::make(ep);
  const uint32_t CR = (uint32_t)ru.CR, RR = (uint32_t)ru.R;
  const uint32_t board = ST(PL_BOARD);
  const uint32_t misc = ST(PL_MISC);
  const int deck_size = (misc >> 8) & 63;
  const uint64_t disc = (uint64_t)ST(PL_DISC_LO) | ((uint64_t)ST(PL_DISC_HI) << 32);
  const uint32_t lastmv = ST(PL_LASTMV);
  const int info = board_info(board), life = board_life(board);
  const uint32_t F = (uint32_t)ep.F;

  for (int p = p_begin; p < P; p += p_step) {
    const uint32_t base = (uint32_t)(lane * P + p) * F;
    const uint32_t pm = ep.shuffle_color ? (ST(PLPERM(p)) & 0x7fffu) : kIdentityPerm;
    if constexpr (FIXED) {
      static_assert(TP > 0 && TH > 0 && !V, "fixed bit positions need a fixed game shape and the full rules");
      uint32_t hand[TP], kcp[TP], krp[TP], kh[TP];
#pragma unroll
      for (int o = 0; o < TP; ++o) {
        int q = p + o;
        if (q >= P) q -= P;
        hand[o] = ST(PLH(q));
        kcp[o] = ST(PLKCP(q));
        krp[o] = ST(PLKRP(q));
        kh[o] = ST(PLKH(q));
      }
      uint32_t row[ObsRowGeom<TP, TH>::NW];
      obs_row_assemble<TP, TH>(row, board, misc, disc, lastmv, greedy_rec, hand, kcp, krp, kh, p, pm, ep.sad != 0);
      obs_row_place<TP, TH>(row, base, ep.sad != 0, [s_obs](uint32_t w, uint32_t v) { atomicOr(&s_obs[w], v); });
    } else {
      uint32_t miss = 0;
#pragma unroll
      for (int o = 0; o < (TP ? TP : 5); ++o) {
        if (o >= P) break;
        int q = p + o;
        if (q >= P) q -= P;
        const uint32_t hw = ST(PLH(q));
        const int len = (hw >> 25) & 7;
        if (len < H) miss |= 1u << o;
        const uint32_t kcp = ST(PLKCP(q)), krp = ST(PLKRP(q)), kh = ST(PLKH(q));
#pragma unroll
        for (int i = 0; i < (TH ? TH : 5); ++i) {
          if (i < len) {
            if (o > 0) {
              const int card = (hw >> (5 * i)) & 31;
              const int c = (card * 13) >> 6, r = card - 5 * c;
              or_bit(s_obs, base + (uint32_t)((o * H + i) * ru.CR) + perm_c(pm, c) * RR + (uint32_t)r);
            }
            const uint32_t cp = (kcp >> (5 * i)) & 31u, rp = (krp >> (5 * i)) & 31u;
            const uint32_t h6 = (kh >> (6 * i)) & 63u;
            uint64_t m = 0;
#pragma unroll
            for (int c = 0; c < 5; ++c) m |= ((cp >> c) & 1u) ? ((uint64_t)rp << (perm_c(pm, c) * RR)) : 0ull;
            if (h6 & 7u) m |= 1ull << (CR + perm_c(pm, (int)(h6 & 7u) - 1));
            if (h6 >> 3) m |= 1ull << (CR + (uint32_t)ru.C + (h6 >> 3) - 1u);
            or_bits64(s_obs, base + (uint32_t)ep.OK + (uint32_t)((o * H + i) * ru.KS), m);
          }
        }
      }
      or_bits32(s_obs, base + (uint32_t)(P * H * ru.CR), miss);
      // board: deck thermometer | fireworks one-hot | info thermometer | life thermometer
      or_bits64(s_obs, base + (uint32_t)ep.OB, (1ull << deck_size) - 1ull);
      uint64_t bm = 0;
#pragma unroll
      for (int c = 0; c < 5; ++c) {
        const int f = board_fw(board, c);
        bm |= (f > 0) ? (1ull << (perm_c(pm, c) * RR + (uint32_t)f - 1u)) : 0ull;
      }
      bm |= (uint64_t)((1u << info) - 1u) << CR;
      bm |= (uint64_t)((1u << life) - 1u) << (CR + (uint32_t)ru.MI);
      or_bits64(s_obs, base + (uint32_t)(ep.OB + ep.DECKW), bm);
      // discards: thermometers of width 3,2,2,2,1 per colour (a variant's R ranks: 3, 2 ... 2, 1; R = 1: 3)
      uint64_t dm = 0;
#pragma unroll
      for (int c = 0; c < 5; ++c) {
        const uint32_t pc = perm_c(pm, c);
#pragma unroll
        for (int r = 0; r < 5; ++r) {
          const uint32_t n = cnt2(disc, c * 5 + r);
          const uint32_t roff = (r == 0) ? 0u : (1u + 2u * (uint32_t)r);
          dm |= (uint64_t)((1u << n) - 1u) << (pc * (uint32_t)ru.DW + roff);
        }
      }
      or_bits64(s_obs, base + (uint32_t)ep.OD, dm);
      or_bits64(s_obs, base + (uint32_t)ep.OL, encode_last_action(P, H, lastmv, p, pm, ru));
      if (ep.sad) or_bits64(s_obs, base + (uint32_t)ep.F0, encode_last_action(P, H, greedy_rec, p, pm, ru));
    }

    const uint64_t lm = legal_mask_of<TH>(P, H, ep.A, s_st, lane, p, pm, ru);
    or_bits64(s_legal, (uint32_t)(lane * P + p) * (uint32_t)ep.A, lm);
    ep.legal_bits[(size_t)g * P + p] = lm;
    if (ep.legal_out) ep.legal_out[(size_t)g * P + p] = lm;
    if (s_lmask) {   // env_rollout_pipe_kernel: where the logic wave's policy reads it in the next iteration (LogicCarry)
      s_lmask[(2 * p) * kWave + lane] = (uint32_t)lm;
      s_lmask[(2 * p + 1) * kWave + lane] = (uint32_t)(lm >> 32);
    }

    // own hand trinary [playable, discardable, other] (EncodeOwnHandTrinary)
    {
      const uint32_t hw = ST(PLH(p));
      const int len = (hw >> 25) & 7;
      uint32_t om = 0;
#pragma unroll
      for (int i = 0; i < (TH ? TH : 5); ++i) {
        const int card = (hw >> (5 * i)) & 31;
        const int c = (card * 13) >> 6, r = card - 5 * c;
        const int f = board_fw(board, c);
        if (i < len) om |= 1u << (3 * i + (r == f ? 0 : (r < f ? 1 : 2)));
      }
      or_bits32(s_own, (uint32_t)(lane * P + p) * (uint32_t)(3 * H), om);
      if (ep.own_bits) ep.own_bits[(size_t)g * P + p] = om;
    }
  }
}

// publicly remaining count of each card type (total - discards - fireworks), 2 bits each
__device__ __forceinline__ uint64_t public_counts(uint64_t disc, uint32_t board, uint64_t full) {
  uint64_t pc = full - disc;  // per-field subtraction never borrows (disc <= total)
#pragma unroll
  for (int c = 0; c < 5; ++c) {
    const int f = board_fw(board, c);
    for (int r = 0; r < f; ++r) pc -= (uint64_t)1 << (2 * (c * 5 + r));
  }
  return pc;
}

// V0-belief fix-up of the knowledge section (knowledge_mode=1): every plausible entry becomes
// count/total as fp32 (EncodeV0Belief in the oracle).  Executed by the whole wave for the games whose
// bit in `active` is set; scattered 4-byte stores over the already streamed 0/1 values.
template <bool V>
__device__ void v0_fixup(const EnvParams& ep, const uint32_t* s_st, const uint32_t* s_obs, uint64_t active, int g0,
                         int lane_id) {
  const int P = ep.P, H = ep.H;
  const auto ru = RulesOf<V>::make(ep);
  const int per_row = P * H * ru.CR;
  while (active) {
    const int lg = __builtin_ctzll(active);
    active &= active - 1;
    const uint32_t board = s_st[PL_BOARD * kWave + lg];
    const uint64_t disc = (uint64_t)s_st[PL_DISC_LO * kWave + lg] | ((uint64_t)s_st[PL_DISC_HI * kWave + lg] << 32);
    const uint64_t pub = public_counts(disc, board, ru.full);
    for (int e = lane_id; e < P * per_row; e += kWave) {
      const int p = e / per_row;
      const int rem = e - p * per_row;
      const int slot = rem / ru.CR;  // o*H + i
      const int j = rem - slot * ru.CR;
      const int o = slot / H, i = slot - o * H;
      int q = p + o;
      if (q >= P) q -= P;
      const uint32_t hw = s_st[PLH(q) * kWave + lg];
      if (i >= (int)((hw >> 25) & 7)) continue;
      const uint32_t bitpos = (uint32_t)(lg * P + p) * (uint32_t)ep.F + (uint32_t)ep.OK + (uint32_t)(slot * ru.KS + j);
      if (!get1(s_obs, bitpos)) continue;
      const uint32_t permw = ep.shuffle_color ? s_st[PLPERM(p) * kWave + lg] : kIdentityPermBoth;
      const uint32_t inv = permw >> 15;
      const uint32_t cp = (s_st[PLKCP(q) * kWave + lg] >> (5 * i)) & 31u;
      const uint32_t rp = (s_st[PLKRP(q) * kWave + lg] >> (5 * i)) & 31u;
      float total = 0.f;
      for (int c = 0; c < 5; ++c)
        if ((cp >> c) & 1u)
          for (int r = 0; r < 5; ++r)
            if ((rp >> r) & 1u) total += (float)cnt2(pub, c * 5 + r);
      const int pcol = j / ru.R, r = j - ru.R * pcol;
      const int real_c = (int)perm_c(inv, pcol);
      const float cnt = (float)cnt2(pub, real_c * 5 + r);
      const float v = (total > 0.f) ? cnt / total : 0.f;
      ep.priv_s[(size_t)(g0 + lg) * P * ep.F + (size_t)p * ep.F + ep.OK + slot * ru.KS + j] = v;
    }
  }
}

__device__ __forceinline__ void log_error(const EnvParams& ep, int g, int code) {
  if (atomicAdd(&ep.err[0], 1u) == 0u) {
    ep.err[1] = (uint32_t)g;
    ep.err[2] = (uint32_t)code;
  }
}

// ---- counter-based random-legal policy ---------------------------------------------------------
// (mix64 and policy_hash: hsad_planes.h)
// k-th set bit of the legal mask, k = hash % popcount (same specification as oracle orc_policy_random)
__device__ __forceinline__ int policy_pick(uint64_t seed, uint64_t game, uint64_t counter, int p, int stream,
                                           uint64_t mask) {
  const uint32_t h = policy_hash(seed, game, counter, (uint64_t)(p * 2 + stream));
  return df_select(mask, h % (uint32_t)__popcll(mask));
}
// The same pick from the hash's inner key, which depends on launch constants only (seed, game, player, stream): a launch that
// keeps its games computes the keys once (env_rollout_pipe_kernel, LogicCarry) and pays one mix64 per pick instead of three.
// nbits: bound on the mask's width (df_select).
__device__ __forceinline__ uint64_t policy_key(uint64_t seed, uint64_t game, int p, int stream) {
  return mix64(seed ^ mix64(game * 0xD1342543DE82EF95ull + (uint64_t)(p * 2 + stream)));
}
__device__ __forceinline__ int policy_pick_keyed(uint64_t key, uint64_t counter, uint64_t mask, int nbits) {
  const uint32_t h = (uint32_t)(mix64(key + counter) >> 32);
  return df_select(mask, h % (uint32_t)__popcll(mask), nbits);
}

// =================================================================================================
// MODE 0: VectorEnv::reset — (re)start every finished/not-started game, rewrite only their rows.
// MODE 1: VectorEnv::step  — apply a[g][cur] (and the SAD greedy move), deal, observe all games.
// MODE 2: MODE 1 with the random-legal policy evaluated in-kernel; the sampled actions are also written to
//         a_out/g_out so the trajectory matches policy kernel + MODE 1.
// MODE 3: the whole thread-loop body in one launch (hsad_env_rollout_random): reset-if-terminated -> policy -> step.
//         Same trajectories as MODE 0 + MODE 2; the observation of a freshly reset state is not materialised
//         (nothing consumes it in the random-policy rollout).
// TP/TH: compile-time players / hand size (0 = run-time values from EnvParams).
// =================================================================================================
constexpr int kEnvThreads = 4 * kWave;  // at most; EnvParams::nthreads (128 | 256) is what a launch uses.  wave 0: game logic; the
                                      // other waves: LDS zeroing; all: row building + streaming

// The workgroup's ng games' rows, LDS -> HBM, by threads [t, t + n) of the workgroup: one contiguous, 16-byte aligned range
// per output tensor (float32 observation, the packed forms when bound, legal moves, own hand)
__device__ __forceinline__ void stream_rows(const EnvParams& ep, const uint32_t* s_obs, const uint32_t* s_legal, const uint32_t* s_own,
                                            int g0, int ng, int P, int H, int t, int n) {
  const size_t PF = (size_t)P * ep.F, PA = (size_t)P * ep.A, PO = (size_t)P * 3 * H;
  if (!ep.obs_f32) {
    // device consumers only: no float32 observation leaves the chip
  } else if (ep.nt_stores) {
    stream_bits_f32_aligned<true>(s_obs, ep.priv_s + (size_t)g0 * PF, (uint32_t)(ng * PF), t, n);
  } else {
    stream_bits_f32_aligned<false>(s_obs, ep.priv_s + (size_t)g0 * PF, (uint32_t)(ng * PF), t, n);
  }
  stream_rows_packed(ep, s_obs, 0, ng * P, (size_t)g0 * P, t, n);
  stream_bits_f32_aligned<false>(s_legal, ep.legal + (size_t)g0 * PA, (uint32_t)(ng * PA), t, n);
  stream_bits_f32_aligned<false>(s_own, ep.own + (size_t)g0 * PO, (uint32_t)(ng * PO), t, n);
}

// The same for the pipelined rollout, whose later streams of a launch reduce the float32 observation to the lines that changed
// (EnvParams::delta).  s_old: the bit rows priv_s was last written from; all: every line (the first stream of a launch, and every
// stream without delta).  The packed forms, legal moves and own hand go out in full from the current rows.  Returns this lane's
// count of observation lines stored (count on: the trace) and, in units, of the units stored (lines, or half lines where the
// stream decided by those).  compact: one wave streams (t its lane, n == kWave) and takes the compacted form where the stream is not
// an `all` stream, by lines (1) or by half lines (2); that form writes its list of changed units into s_old, which the caller
// clears afterwards anyway.  The choice is wave-uniform and made once per stream.  Mixing units within a launch is safe: after any
// stream priv_s equals the rows streamed, whichever unit decided what to skip.
__device__ __forceinline__ unsigned stream_rows_delta(const EnvParams& ep, const uint32_t* s_obs, uint32_t* s_old, bool all,
                                                      const uint32_t* s_legal, const uint32_t* s_own, int g0, int ng, int P, int H,
                                                      int t, int n, bool count, int compact, unsigned& units) {
  const size_t PF = (size_t)P * ep.F, PA = (size_t)P * ep.A, PO = (size_t)P * 3 * H;
  unsigned stored = 0;
  bool by_lines = true;
  if (!ep.obs_f32) {
    // device consumers only: no float32 observation leaves the chip
  } else if (compact && !all) {
    by_lines = false;
    float* out = ep.priv_s + (size_t)g0 * PF;
    if (compact == 2) {
      if (ep.nt_stores) {
        stored = stream_bits_f32_compact<true, 16>(s_obs, s_old, out, (uint32_t)(ng * PF), t, units);
      } else {
        stored = stream_bits_f32_compact<false, 16>(s_obs, s_old, out, (uint32_t)(ng * PF), t, units);
      }
    } else if (ep.nt_stores) {
      stored = stream_bits_f32_compact<true, 32>(s_obs, s_old, out, (uint32_t)(ng * PF), t, units);
    } else {
      stored = stream_bits_f32_compact<false, 32>(s_obs, s_old, out, (uint32_t)(ng * PF), t, units);
    }
  } else if (ep.nt_stores) {
    stored = stream_bits_f32_delta<true>(s_obs, s_old, all, ep.priv_s + (size_t)g0 * PF, (uint32_t)(ng * PF), t, n, count);
  } else {
    stored = stream_bits_f32_delta<false>(s_obs, s_old, all, ep.priv_s + (size_t)g0 * PF, (uint32_t)(ng * PF), t, n, count);
  }
  if (by_lines) units = stored;
  stream_rows_packed(ep, s_obs, 0, ng * P, (size_t)g0 * P, t, n);
  stream_bits_f32_aligned<false>(s_legal, ep.legal + (size_t)g0 * PA, (uint32_t)(ng * PA), t, n);
  stream_bits_f32_aligned<false>(s_own, ep.own + (size_t)g0 * PO, (uint32_t)(ng * PO), t, n);
  return stored;
}

// zero `nz` LDS words from p (16-byte aligned) by threads [t, t + n)
__device__ __forceinline__ void clear_words(uint32_t* p, int nz, int t, int n) {
  uint4* z4 = reinterpret_cast<uint4*>(p);
  for (int k = t; k < (nz >> 2); k += n) z4[k] = make_uint4(0u, 0u, 0u, 0u);
  for (int k = (nz & ~3) + t; k < nz; k += n) p[k] = 0u;
}

// zero the obs / legal / own bit rows (contiguous in LDS from s_obs) by threads [t, t + n)
__device__ __forceinline__ void clear_rows(const EnvParams& ep, uint32_t* s_obs, int t, int n) {
  const int nz = ep.obs_words + ep.legal_words + ep.own_words;
  uint4* z4 = reinterpret_cast<uint4*>(s_obs);
  for (int k = t; k < (nz >> 2); k += n) z4[k] = make_uint4(0u, 0u, 0u, 0u);
  for (int k = (nz & ~3) + t; k < nz; k += n) s_obs[k] = 0u;
}

// What env_rollout_pipe_kernel holds on to from one iteration of a launch to the next instead of going through global memory for
// it (env_logic<..., CARRY = true>; every other caller passes none and compiles the statements it always had: counter and masks
// are read from, and the counter written to, global memory every time).
//   counter: this lane's act counter (EnvParams::act_count), loaded in the launch's prologue and stored after its last iteration.
//   s_lmask: the legal masks build_rows left in LDS in phase B of the previous iteration, mask of (lane, p) as two words at
//            [(2p) * kWave + lane] and [(2p + 1) * kWave + lane] of the lane's own column of the mt19937 prefetch window.  A lane
//            uses that column only in an iteration in which its game restarts, and then recomputes its masks from the fresh state,
//            so the two never meet; the words cost no LDS.  The launch's prologue fills them from EnvParams::legal_bits: nothing is
//            assumed about what ran before the launch.  (Every window holds 2PH + P + 2 words or more per lane, hsad_env_create.)
//   pkey:    this lane's policy keys (policy_key of player p, stream s at [2p + s]), computed in the launch's prologue: game, seed,
//            player and stream do not change during a launch.  Only in the instances kPolicyKeys names (two registers per key; the
//            others have none to spare without scratch) -- elsewhere nullptr and never read.
struct LogicCarry {
  uint32_t* counter;
  const uint32_t* s_lmask;
  const uint64_t* pkey;
};
template <int TP, int TH>
constexpr bool kPolicyKeys = (TP == 2 && TH == 5);
// key i of N: constant indices only, so the keys stay in registers whether or not the loop over the players is unrolled
template <int N>
__device__ __forceinline__ uint64_t carried_key(const uint64_t* k, int i) {
  uint64_t v = k[0];
#pragma unroll
  for (int j = 1; j < N; ++j) v = (i == j) ? k[j] : v;
  return v;
}
typedef __attribute__((address_space(3))) const uint32_t* LdsWordPtr;   // a load through it is an LDS instruction, never a flat one

// The game logic of one iteration for the 64 games of the logic wave (wave 0): reset-if-terminated (MODE 0 / 3), then the
// policy (MODE 2 / 3) or the given actions (MODE 1) and the env step, all on the state planes staged in s_st.
template <int MODE, int TP, int TH, bool V = false, class EP = EnvParams, bool CARRY = false>
__device__ __forceinline__ void env_logic(const EP& ep, const int64_t* __restrict__ a_in, const int64_t* __restrict__ g_in,
                                          uint32_t* s_st, uint32_t* s_win, const float* s_eps, const int lane, const int g,
                                          const bool active, const bool do_reset, Rng& rng, uint32_t& greedy_rec, float& reward,
                                          bool& term, const int dbg_it = 0, const LogicCarry carry = {nullptr, nullptr, nullptr}) {
  const int P = TP ? TP : ep.P, H = TH ? TH : ep.H;
  const auto ru = RulesOf<V>::make(ep);
  if (MODE == 0 || MODE == 3) {
    // ---- prefetch window: every mt19937 word this reset will regenerate, in one round trip ----
    const int W = ep.win_w;
    // what hsad_env_create can set W to in this instance: 2PH + P + 2 draws of a reset, with shuffle_color 1 + 2 (P - 1) more, 64 at most
    constexpr int kWmin = (TP && !V) ? (2 * TP * TH + TP + 2 < 64 ? 2 * TP * TH + TP + 2 : 64) : 0;
    constexpr int kWmax = (TP && !V) ? (kWmin + 1 + 2 * (TP - 1) < 64 ? kWmin + 1 + 2 * (TP - 1) : 64) : 64;
    constexpr int kNB = kWmax <= 32 ? kWmax : 32;   // words of the one-batch form
    uint32_t* winA = s_win + lane;                   // x[wbase + k],       k in [0, W]   (W > 32 only)
    uint32_t* winB = s_win + (W <= 32 ? 0 : (W + 1) * kWave) + lane;  // x[wbase + k + 397], k in [0, W) -> new words
    const uint32_t wbase = rng.spos;
    if (do_reset) {
      if (kWmax <= 32 || (kWmin <= 32 && W <= 32)) {
        // one batch: all 2 kNB + 1 words in flight together, regenerated in registers, only the new words go to LDS.  wbase < 624
        // and j + 397 < 624, so an index wraps at most once: the lane's base pointer or the one 624 words below it, and the
        // word's offset in the instruction (words past W are real state words, loaded and left unused)
        const uint32_t* pw = rng.mt + wbase;
        const uint32_t* pw_wrapped = pw - kMtN;
        const int n0 = kMtN - (int)wbase;   // the first j for which wbase + j wraps
        uint32_t va[kNB + 1], vb[kNB];
#pragma unroll
        for (int j = 0; j <= kNB; ++j) va[j] = (j >= n0 ? pw_wrapped : pw)[j];
#pragma unroll
        for (int j = 0; j < kNB; ++j) vb[j] = (j >= n0 - kMtM ? pw_wrapped : pw)[j + kMtM];
#pragma unroll
        for (int j = 0; j < kNB; ++j)
          if (j < kWmin || j < W) winB[j * kWave] = mt_twist(va[j], va[j + 1], vb[j]);
      } else {
        for (int k0 = 0; k0 <= W; k0 += 16) {
          uint32_t va[16], vb[16];
#pragma unroll
          for (int j = 0; j < 16; ++j) {
            const uint32_t k = (uint32_t)min(k0 + j, W);
            va[j] = rng.mt[(wbase + k) % (uint32_t)kMtN];
            vb[j] = rng.mt[(wbase + k + kMtM) % (uint32_t)kMtN];
          }
#pragma unroll
          for (int j = 0; j < 16; ++j)
            if (k0 + j <= W) {
              winA[(k0 + j) * kWave] = va[j];
              if (k0 + j < W) winB[(k0 + j) * kWave] = vb[j];
            }
        }
        for (int k = 0; k < W; ++k) winB[k * kWave] = mt_twist(winA[k * kWave], winA[(k + 1) * kWave], winB[k * kWave]);
      }
      STAMP(6);
      rng.win = winB;
      rng.w_n = W;
      rng.spos = df_wrap624(wbase, (uint32_t)W);

      // HanabiEnv::reset (cpp/hanabi_env.cc:9-47): fresh HanabiState, deal until no chance node
      const uint64_t deck = ru.full;
      ST(PL_DECK_LO) = (uint32_t)deck;
      ST(PL_DECK_HI) = (uint32_t)(deck >> 32);
      ST(PL_DISC_LO) = 0;
      ST(PL_DISC_HI) = 0;
      ST(PL_BOARD) = ((uint32_t)ru.MI << 15) | ((uint32_t)ru.ML << 19) | ((uint32_t)P << 21) | (0u << 24) | (0u << 27);
      ST(PL_MISC) = (ST(PL_MISC) & (63u << 16)) | ((uint32_t)ru.deck << 8) | (1u << 15);  // keep last_score; started
      ST(PL_LASTMV) = 0;
      {
        // initial deal (ApplyRandomChance until every hand is full: players in seat order, H cards each) with the
        // deck and the hand being filled held in registers — one LDS store per plane at the end instead of ~35
        // dependent LDS round trips per card
        uint64_t dk = deck;
        int dsize = ru.deck;
        const uint32_t full_k = (H >= 5) ? 0x1ffffffu : ((1u << (5 * H)) - 1u);
        uint32_t full_kc = full_k, full_kr = full_k;   // every colour / rank plausible in each of the H slots
        if (V) {
          full_kc = full_kr = 0u;
          for (int i = 0; i < H; ++i) {
            full_kc |= ru.cmask << (5 * i);
            full_kr |= ru.rmask << (5 * i);
          }
        }
        if constexpr (TP > 0 && !V) {
          // The full deck keeps two card types or more while these P H <= 20 cards leave it, so the deal takes exactly 2 P H
          // draws, and they are known in advance: the buffered look-ahead outputs first (la_n of them), then the window's words
          // in order (it holds 2PH + P + 2 or more).  No generator call, no branch on where a draw comes from; card k leaves a
          // deck of 50 - k.  The pick is deal_pick's: the bounded search inside the band, the literal restatement outside it and
          // under deal_mode 1.  The generator's bookkeeping is set afterwards to what 2 P H calls of rng_next leave.
          const int la_start = rng.la_n;
          int wpos = -la_start;   // window word of the next draw (below 0: a look-ahead output)
          uint32_t dleft = (uint32_t)ru.deck;
#pragma clang loop unroll(disable)
          for (int p = 0; p < P; ++p) {
            uint32_t hw = 0;
#pragma clang loop unroll(disable)
            for (int i = 0; i < H; ++i) {
              uint32_t u1 = mt_temper(winB[max(wpos, 0) * kWave]);
              uint32_t u2 = mt_temper(winB[max(wpos + 1, 0) * kWave]);
              if (wpos < 0) {   // the first card only
                u1 = rng.la0;
                if (wpos < -1) u2 = rng.la1;
              }
              wpos += 2;
              const uint64_t p0 = (uint64_t)u1 * dleft, p1 = (uint64_t)u2 * dleft + (p0 >> 32);   // (u1 + 2^32 u2) dleft, 96 bits
              const uint64_t lo = (uint64_t)(uint32_t)p0 | (p1 << 32);
              int t;
              if (ep.deal_mode == 0 && lo >= (1ull << 28) && lo <= 0ull - (1ull << 28))
                t = df_pick(dk, (uint32_t)(p1 >> 32) + 1u);
              else
                t = deal_pick_exact(dk, (int)dleft, u1, u2);
              dk -= (uint64_t)1 << (2 * t);
              if (ep.track_dh) ep.deck_hist[(size_t)g * 52 + (ru.deck - (int)dleft)] = (uint8_t)t;
              dleft -= 1u;
              hw |= (uint32_t)t << (5 * i);
            }
            ST(PLH(p)) = hw | ((uint32_t)H << 25);
            ST(PLKCP(p)) = full_kc;
            ST(PLKRP(p)) = full_kr;
            ST(PLKH(p)) = 0;
          }
          dsize = (int)dleft;
          rng.draws += (uint32_t)(2 * P * H);
          if (la_start > 0) rng.la0 = rng.la1;
          rng.la_n = 0;
          rng.w_c = 2 * P * H - la_start;
        } else {
          for (int p = 0; p < P; ++p) {
            uint32_t hw = 0;
            for (int i = 0; i < H; ++i) {
              const int t = deal_pick(ep.deal_mode, dk, dsize, rng);
              dk -= (uint64_t)1 << (2 * t);
              if (ep.track_dh) ep.deck_hist[(size_t)g * 52 + (ru.deck - dsize)] = (uint8_t)t;
              dsize -= 1;
              hw |= (uint32_t)t << (5 * i);
            }
            ST(PLH(p)) = hw | ((uint32_t)H << 25);
            ST(PLKCP(p)) = full_kc;
            ST(PLKRP(p)) = full_kr;
            ST(PLKH(p)) = 0;
          }
        }
        ST(PL_DECK_LO) = (uint32_t)dk;
        ST(PL_DECK_HI) = (uint32_t)(dk >> 32);
        ST(PL_MISC) = (ST(PL_MISC) & ~(63u << 8)) | ((uint32_t)dsize << 8);
        // all hands full -> AdvanceToNextPlayer leaves the chance node: cur = 0, next = 1 % P
        ST(PL_BOARD) = board_set(board_set(ST(PL_BOARD), 24, 7u, 1u), 27, 7u, (uint32_t)(1 % P));
      }
      STAMP(7);
      for (int p = 0; p < P; ++p) {
        const uint32_t r = rng_next(rng) % (uint32_t)ep.n_eps;
        // (CARRY: the staged list through an LDS pointer and the rest behind a branch; the select of the two addresses is a
        // flat load, which is waited for on the vector-memory counter as well, i.e. behind the wave's stores)
        if (!CARRY) {
          ST(PLEPS(p)) = __float_as_uint(r < 128u ? s_eps[r] : ep.eps_list[r]);
        } else {
          uint32_t e;
          if (r < 128u)
            e = ((LdsWordPtr)reinterpret_cast<const uint32_t*>(s_eps))[r];
          else
            e = __float_as_uint(ep.eps_list[r]);
          ST(PLEPS(p)) = e;
        }
      }
      if (ep.shuffle_color) {
        const int fix = (int)(rng_next(rng) % (uint32_t)P);
        for (int p = 0; p < P; ++p) {
          uint32_t arr = kIdentityPerm;
          auto swp = [&](int i, int j) {
            const uint32_t vi = (arr >> (3 * i)) & 7u, vj = (arr >> (3 * j)) & 7u;
            arr = (arr & ~(7u << (3 * i))) | (vj << (3 * i));
            arr = (arr & ~(7u << (3 * j))) | (vi << (3 * j));
          };
          if (V && p != fix) {
            // libstdc++ std::shuffle of C colours: an even C swaps slot 1 first on a {0, 1} draw, then two swaps per
            // uniform_int draw over [0, (i+1)(i+2)) (C = 1 draws nothing); positions C..4 stay the identity
            int i = 1;
            if ((ru.C & 1) == 0) {
              swp(1, (int)uniform_below(2u, rng));
              i = 2;
            }
            for (; i + 1 < ru.C; i += 2) {
              const uint32_t b1 = (uint32_t)i + 2u;
              const uint32_t x = uniform_below((uint32_t)(i + 1) * b1, rng);
              swp(i, (int)(x / b1));
              swp(i + 1, (int)(x % b1));
            }
          } else if (p != fix) {
            // libstdc++ std::shuffle, 5 elements: two swaps per uniform_int draw
            uint32_t x = uniform_below(6u, rng);
            swp(1, (int)(x / 3u));
            swp(2, (int)(x % 3u));
            x = uniform_below(20u, rng);
            swp(3, (int)(x / 5u));
            swp(4, (int)(x % 5u));
          }
          uint32_t inv = 0;
          for (int i = 0; i < 5; ++i) inv |= (uint32_t)i << (3 * ((arr >> (3 * i)) & 7u));
          ST(PLPERM(p)) = arr | (inv << 15);
        }
      } else {
        for (int p = 0; p < P; ++p) ST(PLPERM(p)) = kIdentityPermBoth;
      }
      // top the look-ahead up from the window, then publish the regenerated words
      while (rng.la_n < 2 && rng.w_c < rng.w_n) {
        la_push(rng, mt_temper(winB[rng.w_c * kWave]));
        rng.w_c += 1;
      }
      uint32_t wi = wbase;
      for (int k = 0; k < rng.w_c; ++k) {
        rng.mt[wi] = winB[k * kWave];
        wi = wrap624(wi + 1u);
      }
      if (rng.w_c < rng.w_n) rng.spos = df_wrap624(wbase, (uint32_t)rng.w_c);
      rng.w_n = rng.w_c;
    }
  }
  if (MODE != 0) {
    if (active) {
      uint32_t misc = ST(PL_MISC);
      const bool started = (misc >> 15) & 1u, was_term = (misc >> 14) & 1u;
      uint32_t board = ST(PL_BOARD);
      const int cur = board_cur(board);
      term = was_term;
      if (!started || was_term || cur < 0) {
        log_error(ep, g, 3);  // assert(!terminated()) in HanabiEnv::step
      } else {
        int uid, guid = 0;
        if (MODE >= 2) {
          uint32_t counter;
          if (CARRY) {
            counter = *carry.counter;
            *carry.counter = counter + 1u;
          } else {
            counter = ep.act_count[g];
            ep.act_count[g] = counter + 1u;
          }
          uid = guid = 0;
          // the greedy stream's pick is read by the SAD step and by a caller that asked for it; nobody else pays for it
          const bool need_g = ep.sad || ep.g_out != nullptr;
          constexpr int kABits = (TP && !V) ? 2 * TH + (TP - 1) * 10 + 1 : 64;   // A of the full game: no legal bit at or above it
          for (int p = 0; p < P; ++p) {
            // legal bits of the state the policy acts on: the stored side output (global memory, or the copy build_rows left
            // in LDS: LogicCarry), or (MODE 3, game restarted a moment ago in this very launch) recomputed from the fresh state
            uint64_t mask;
            if (CARRY) {   // (a compile-time choice: chosen at run time, the global load and its vmcnt(0) at the join stay in the loop)
              if (do_reset) {
                mask = legal_mask_of<TH>(P, H, ep.A, s_st, lane, p, ep.shuffle_color ? (ST(PLPERM(p)) & 0x7fffu) : kIdentityPerm, ru);
              } else {
                const LdsWordPtr lm = (LdsWordPtr)carry.s_lmask;
                mask = (uint64_t)lm[(2 * p) * kWave + lane] | ((uint64_t)lm[(2 * p + 1) * kWave + lane] << 32);
              }
            } else {
              mask = do_reset ? legal_mask_of<TH>(P, H, ep.A, s_st, lane, p,
                                                  ep.shuffle_color ? (ST(PLPERM(p)) & 0x7fffu) : kIdentityPerm, ru)
                              : ep.legal_bits[(size_t)g * P + p];
            }
            int pa, pg = 0;
            if constexpr (CARRY && kPolicyKeys<TP, TH>) {
              pa = policy_pick_keyed(carried_key<2 * TP>(carry.pkey, 2 * p), (uint64_t)counter, mask, kABits);
              if (need_g) pg = policy_pick_keyed(carried_key<2 * TP>(carry.pkey, 2 * p + 1), (uint64_t)counter, mask, kABits);
            } else {
              pa = policy_pick(ep.policy_seed, (uint64_t)g, (uint64_t)counter, p, 0, mask);
              if (need_g) pg = policy_pick(ep.policy_seed, (uint64_t)g, (uint64_t)counter, p, 1, mask);
            }
            ep.a_out[(size_t)g * P + p] = pa;
            if (ep.g_out) ep.g_out[(size_t)g * P + p] = pg;
            if (p == cur) {
              uid = pa;
              guid = pg;
            }
          }
        } else {
          uid = (int)a_in[(size_t)g * P + cur];
          if (ep.sad) guid = (int)g_in[(size_t)g * P + cur];
        }
        MoveDec mv = decode_uid(uid, P, H, ru);
        const uint32_t pinv = ep.shuffle_color ? (ST(PLPERM(cur)) >> 15) : kIdentityPerm;
        if (mv.type == 3) mv.val = (int)perm_c(pinv, mv.val);  // maybeInversePermuteColor_
        bool ok = move_is_legal(P, s_st, lane, mv, ru);
        if (!ok) log_error(ep, g, 1);
        if (ok && ep.sad) {
          MoveDec gm = decode_uid(guid, P, H, ru);
          if (gm.type == 3) gm.val = (int)perm_c(pinv, gm.val);
          if (!move_is_legal(P, s_st, lane, gm, ru)) {
            ok = false;
            log_error(ep, g, 2);
          } else {
            greedy_rec = make_history(P, s_st, lane, gm, ru);
          }
        }
        if (ok) {
          const int num_step = (int)(misc & 255u) + 1;
          const int deck_size = (misc >> 8) & 63;
          const int life0 = board_life(board);
          const int prev_score = (life0 <= 0 && ep.bomb) ? 0 : board_fw_sum(board);
          const uint32_t rec = make_history(P, s_st, lane, mv, ru);
          // ---- HanabiState::ApplyMove ----
          if (deck_size == 0) board = board_set(board, 21, 7u, (uint32_t)(board_turns(board) - 1));
          if (mv.type <= 2) {
            const uint32_t hw = ST(PLH(cur));
            const int len = (hw >> 25) & 7;
            const int card = (hw >> (5 * mv.idx)) & 31;
            const int c = (card * 13) >> 6, r = card - 5 * c;
            bool to_discard = true;
            if (mv.type == 2) {
              if ((rec >> 30) & 1u) board = board_set(board, 15, 15u, (uint32_t)(board_info(board) + 1));
            } else {
              if ((rec >> 29) & 1u) {
                board = board_set(board, 3 * c, 7u, (uint32_t)(r + 1));
                if ((rec >> 30) & 1u) board = board_set(board, 15, 15u, (uint32_t)(board_info(board) + 1));
                to_discard = false;
              } else {
                board = board_set(board, 19, 3u, (uint32_t)(life0 - 1));
              }
            }
            if (to_discard) {
              uint64_t disc = (uint64_t)ST(PL_DISC_LO) | ((uint64_t)ST(PL_DISC_HI) << 32);
              disc += (uint64_t)1 << (2 * card);
              ST(PL_DISC_LO) = (uint32_t)disc;
              ST(PL_DISC_HI) = (uint32_t)(disc >> 32);
            }
            uint32_t nh = remove_field(hw, mv.idx, 5, 5);
            nh = (nh & ~(7u << 25)) | ((uint32_t)(len - 1) << 25);
            ST(PLH(cur)) = nh;
            ST(PLKCP(cur)) = remove_field(ST(PLKCP(cur)), mv.idx, 5, 5);
            ST(PLKRP(cur)) = remove_field(ST(PLKRP(cur)), mv.idx, 5, 5);
            ST(PLKH(cur)) = remove_field(ST(PLKH(cur)), mv.idx, 6, 5);
          } else {
            board = board_set(board, 15, 15u, (uint32_t)(board_info(board) - 1));
            int q = cur + mv.off;
            if (q >= P) q -= P;
            const uint32_t hw = ST(PLH(q));
            const int len = (hw >> 25) & 7;
            const uint32_t match = (rec >> 18) & 31u;
            const int kpl = (mv.type == 3) ? PLKCP(q) : PLKRP(q);
            uint32_t kp = ST(kpl);
            uint32_t kh = ST(PLKH(q));
            const int hshift = (mv.type == 3) ? 0 : 3;
#pragma unroll
            for (int i = 0; i < 5; ++i) {
              if (i < len) {
                if ((match >> i) & 1u) {
                  kp = (kp & ~(31u << (5 * i))) | ((1u << mv.val) << (5 * i));
                  kh = (kh & ~(7u << (6 * i + hshift))) | ((uint32_t)(mv.val + 1) << (6 * i + hshift));
                } else {
                  kp &= ~((1u << mv.val) << (5 * i));
                }
              }
            }
            ST(kpl) = kp;
            ST(PLKH(q)) = kh;
          }
          ST(PL_LASTMV) = rec;
          board = advance_player(P, H, s_st, lane, board, deck_size);
          ST(PL_BOARD) = board;
          // ---- HanabiEnv::step tail (cpp/hanabi_env.cc:94-108) ----
          const int life1 = board_life(board);
          const int fsum = board_fw_sum(board);
          term = (life1 < 1) || (fsum >= ru.CR) || (board_turns(board) <= 0);
          const int score = (life1 <= 0 && ep.bomb) ? 0 : fsum;
          reward = (float)(score - prev_score);
          if (ep.max_len > 0 && num_step == ep.max_len) {
            term = true;
            reward = (float)(0 - prev_score);
          }
          misc = (misc & ~255u) | (uint32_t)num_step;
          ST(PL_MISC) = misc;
          if (!term) {
            while (board_cur(ST(PL_BOARD)) < 0) deal_one(ep, P, H, s_st, lane, rng, g, ru);
          }
          misc = ST(PL_MISC);
          misc = (misc & ~(1u << 14)) | ((term ? 1u : 0u) << 14);
          if (term) misc = (misc & ~(63u << 16)) | ((uint32_t)(score + 1) << 16);  // lastScore_ (hanabi_env.h:92-94)
          ST(PL_MISC) = misc;
        }
      }
    }
  }
}

template <int MODE, int TP, int TH, bool V = false, class EP = EnvParams>
__device__ __forceinline__ void env_body(const EP& ep, const int64_t* __restrict__ a_in, const int64_t* __restrict__ g_in,
                                         const int g_bias = 0, const int dbg_it = 0) {
  extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
  uint32_t* s_st = smem;
  uint32_t* s_obs = s_st + ep.npl * kWave;
  uint32_t* s_legal = s_obs + ep.obs_words;
  uint32_t* s_own = s_legal + ep.legal_words;
  uint32_t* s_win = s_own + ep.own_words;  // reset kernel only: [win_words][kWave]
  uint32_t* s_grec = s_win + (MODE == 0 || MODE == 3 ? ep.win_words * kWave : 0);  // [kWave] SAD greedy records
  float* s_eps = reinterpret_cast<float*>(s_grec + kWave);  // [min(n_eps, 128)] copy of the eps list (reset only)

  const int tid = threadIdx.x;
  const int lane = tid & (kWave - 1);
  const int wave = tid >> 6;
  const int nthreads = ep.nthreads, nwaves = nthreads >> 6;
  const int g0 = ep.g_begin + blockIdx.x * ep.gpw + g_bias;   // g_bias: always 0 (see env_rollout_kernel)
  const int g = g0 + lane;
  const bool valid = lane < ep.gpw && g < ep.G;
  const int ng = min(ep.gpw, ep.G - g0);
  if (ng <= 0) return;   // 32-game workgroups: the padded game count (a multiple of 64) may add a whole empty workgroup
  const int P = TP ? TP : ep.P, H = TH ? TH : ep.H;

  if (MODE == 3 && ep.phase) {
    if (blockIdx.x == 0 && tid == 0) {   // announce this launch (time first, then the tag that validates it)
      __hip_atomic_store(ep.phase + 2 * ep.part + 1, (unsigned long long)wall_clock64(), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_store(ep.phase + 2 * ep.part, ep.launch_tag, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
    }
    if (ep.n_part > 1 && ep.lock_ticks > 0 && lane == 0) {
      // ring order A(i), B(i), ..., A(i+1): wait for the predecessor's launch (same iteration, or the previous one for
      // partition 0) to have STARTED lock_ticks ago.  If the predecessor is already further along, or silent for 200 us,
      // just go: the lock is an optimisation, never a dependency.
      const int pred = (ep.part + ep.n_part - 1) % ep.n_part;
      const unsigned long long want = ep.part > 0 ? ep.launch_tag : ep.launch_tag - 1ull;
      const unsigned long long t_in = wall_clock64();
      while (want >= ep.first_tag && wall_clock64() - t_in < 20000ull) {
        const unsigned long long tg = __hip_atomic_load(ep.phase + 2 * pred, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT);
        if (tg > want) break;                        // predecessor already ahead: nothing to align with
        if (tg == want) {
          const unsigned long long ref = __hip_atomic_load(ep.phase + 2 * pred + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          while ((long long)(wall_clock64() - ref) < (long long)ep.lock_ticks && wall_clock64() - t_in < 20000ull)
            __builtin_amdgcn_s_sleep(8);
          break;
        }
        __builtin_amdgcn_s_sleep(8);
      }
    }
  }
  STAMP_START();
  const uint32_t misc0 = ep.planes[(size_t)PL_MISC * ep.Gpad + g];
  bool active;
  const bool needs_reset = valid && (!((misc0 >> 15) & 1u) || ((misc0 >> 14) & 1u));
  if (MODE == 0) {
    active = needs_reset;
    if (__ballot(active) == 0ull) return;
  } else {
    active = valid;
  }
  const bool do_reset = (MODE == 0 || MODE == 3) && needs_reset;
  // wave 0 stages all state planes in LDS (loads issued in batches of 8 so they overlap);
  // wave 1 meanwhile clears the bit-row buffers
  if (wave == 0) {
    for (int pl0 = 0; pl0 < ep.npl; pl0 += 8) {
      uint32_t v[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = ep.planes[(size_t)min(pl0 + j, ep.npl - 1) * ep.Gpad + g];
#pragma unroll
      for (int j = 0; j < 8; ++j)
        if (pl0 + j < ep.npl) ST(pl0 + j) = v[j];
    }
  } else {
    const int zt = tid - kWave, zn = nthreads - kWave;            // the clearing waves' thread index / count
    clear_rows(ep, s_obs, zt, zn);
    if (MODE == 0 || MODE == 3)
      for (int k = zt; k < min(ep.n_eps, 128); k += zn) s_eps[k] = ep.eps_list[k];
  }
  __syncthreads();
  STAMP(1);

  Rng rng;
  rng.mt = ep.mt + (size_t)g * kMtN;
  rng.draws = ST(PL_DRAWS);
  rng.la0 = ST(PL_LA0);
  rng.la1 = ST(PL_LA1);
  rng.la_n = (int)((ST(PL_MISC) >> 22) & 3u);
  rng.spos = (rng.draws + (uint32_t)rng.la_n) % (uint32_t)kMtN;
  rng.win = nullptr;
  rng.w_c = rng.w_n = 0;
  uint32_t greedy_rec = 0;
  float reward = 0.f;
  bool term = false;

  if (wave == 0) {
    env_logic<MODE, TP, TH, V>(ep, a_in, g_in, s_st, s_win, s_eps, lane, g, active, do_reset, rng, greedy_rec, reward, term, dbg_it);
    s_grec[lane] = greedy_rec;
  }
  __syncthreads();
  STAMP(2);

  // look-ahead refill (wave 0): loads go out now and are consumed after the rows are built
  Refill rf;
  refill_issue(rf, rng, active && wave == 0);
  // both waves build rows: wave w takes observers w, w+2, ...
  if (active) build_rows<TP, TH, V>(ep, s_st, lane, g, s_obs, s_legal, s_own, s_grec[lane], wave, nwaves);
  STAMP(3);
  if (active && wave == 0) {
    refill_finish(rf, rng);
    ST(PL_DRAWS) = rng.draws;
    ST(PL_LA0) = rng.la0;
    ST(PL_LA1) = rng.la1;
    ST(PL_MISC) = (ST(PL_MISC) & ~(3u << 22)) | ((uint32_t)rng.la_n << 22);
    // write state back (coalesced per plane)
    for (int pl = 0; pl < ep.npl; ++pl) ep.planes[(size_t)pl * ep.Gpad + g] = ST(pl);
  }
  __syncthreads();
  STAMP(4);

  const size_t PF = (size_t)P * ep.F, PA = (size_t)P * ep.A, PO = (size_t)P * 3 * H;
  if (MODE >= 1) {
    stream_rows(ep, s_obs, s_legal, s_own, g0, ng, P, H, tid, nthreads);
    if (valid && wave == 0) {
      for (int p = 0; p < P; ++p) ep.eps[(size_t)g * P + p] = __uint_as_float(ST(PLEPS(p)));
      ep.reward[g] = reward;
      ep.terminal[g] = term ? 1 : 0;
    }
    if (ep.kmode == 1) {
      __syncthreads();
      if (wave == 0) v0_fixup<V>(ep, s_st, s_obs, __ballot(valid), g0, lane);
    }
  } else {
    if (wave != 0) return;  // the reset kernel streams a handful of games per block: one wave is plenty
    uint64_t todo = __ballot(active);
    const uint64_t todo_all = todo;
    while (todo) {
      const int lg = __builtin_ctzll(todo);
      todo &= todo - 1;
      if (ep.obs_f32) stream_bits_f32(s_obs, (uint32_t)(lg * PF), ep.priv_s + (size_t)(g0 + lg) * PF, (uint32_t)PF, lane);
      stream_rows_packed(ep, s_obs, lg * P, P, (size_t)(g0 + lg) * P, lane, kWave);
      stream_bits_f32(s_legal, (uint32_t)(lg * PA), ep.legal + (size_t)(g0 + lg) * PA, (uint32_t)PA, lane);
      stream_bits_f32(s_own, (uint32_t)(lg * PO), ep.own + (size_t)(g0 + lg) * PO, (uint32_t)PO, lane);
    }
    if (active)
      for (int p = 0; p < P; ++p) ep.eps[(size_t)g * P + p] = __uint_as_float(ST(PLEPS(p)));
    if (ep.kmode == 1) {
      __syncthreads();
      v0_fixup<V>(ep, s_st, s_obs, todo_all, g0, lane);
    }
  }
  STAMP(5);
}

// V: a variant's rules from EnvParams (generic players / hand size only); the full game's instances have V = false
template <int MODE, int TP, int TH, bool V = false>
__global__ __launch_bounds__(kEnvThreads) void env_kernel(EnvParams ep, const int64_t* __restrict__ a_in,
                                                          const int64_t* __restrict__ g_in) {
  env_body<MODE, TP, TH, V>(ep, a_in, g_in);
}

// the step (MODE 1) of an env that holds a deal script: next_card reads it.  A kernel of its own, so that env_kernel is compiled
// from what it always was
template <int TP, int TH, bool V = false>
__global__ __launch_bounds__(kEnvThreads) void env_step_scripted_kernel(ScriptedParams ep, const int64_t* __restrict__ a_in,
                                                                        const int64_t* __restrict__ g_in) {
  env_body<1, TP, TH, V>(ep, a_in, g_in);
}

// Persistent rollout: games are independent, so a workgroup simply runs n_iter iterations (reset finished games + policy +
// step + observe) for its 64 games without meeting the others at launch boundaries.  Workgroups that share a CU drift
// apart (and are started apart: stagger_ticks), so one's game-logic phase overlaps the others' observation streams and HBM
// sees a steady write stream -- what the phase-locked partitions approximate with three launches per iteration.
// g_bias is an opaque zero: with a loop-invariant game index the compiler hoists every per-lane address of the body out of
// the loop and ends up at 258 VGPRs (95 without the loop), i.e. one wave per SIMD instead of five.
__device__ __forceinline__ void rollout_stagger(const EnvParams& ep) {
  if (ep.stagger_ticks > 0) {
    // which workgroups start late: (mode 0, rounds 1-5) by XCD = block id mod 8; (1) by block-id group of 32 inside the XCD -- the workgroups
    // that share a CU when the dispatcher walks the XCD's CUs breadth first; (2) by block id inside the XCD mod 4 -- the same when it fills a
    // CU first; (3) by the wave slot the hardware reports (HW_ID wave id bits: whatever the dispatcher did)
    unsigned k = blockIdx.x & 7u;
    if (ep.stagger_mode == 1) k = ((blockIdx.x >> 3) >> 5) & 3u;
    else if (ep.stagger_mode == 2) k = (blockIdx.x >> 3) & 3u;
    else if (ep.stagger_mode == 3) {
      unsigned hw;
      asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
      k = (hw & 15u) >> 1;      // wave id inside the SIMD (2 waves of a workgroup per SIMD pair... see the probe's printout)
    }
    const unsigned long long t_in = wall_clock64(), wait = (unsigned long long)k * (unsigned long long)ep.stagger_ticks;
    while (wall_clock64() - t_in < wait) __builtin_amdgcn_s_sleep(16);
  }
}

// Pacing of a persistent launch.  The observation streams are limited by contention for HBM, not by the CU: a stream takes about
// as long as there are workgroups streaming at once.  Workgroups run at persistently different rates, so the launch ends on the
// slowest while the fastest have long left.  A workgroup that is ahead of the mean therefore holds its stream back and leaves the
// bandwidth to the others.  Nothing is handed over and nobody waits for anybody: each workgroup reads one shared counter and
// sleeps a bounded time that depends on nothing else, so results cannot change and a launch can only end on the workgroup it
// would have ended on anyway.
//   s        what the workgroup's fetch_add of iteration `iter` returned: iteration starts of the whole launch so far + pace_base
//   lead     iter - (s - pace_base) / pace_blocks: iterations this workgroup is ahead of the mean (fixed point, 8 fractional bits)
//   delay    (lead - L0) * t_own, at most min(t_own / 2, pace_cap_ticks); t_own = the workgroup's own last iteration time.
//            The dead band L0 and the proportional form mean that a workgroup never sleeps itself behind the mean.
// A lead outside [-n_iter, n_iter] cannot come from this launch (a stale base, hsad_env_debug_pace_bias): no delay.
__device__ __forceinline__ unsigned pace_delay(const EnvParams& ep, unsigned long long s, int iter, unsigned t_own) {
  const long long num = (long long)iter * ep.pace_blocks - (long long)(s - ep.pace_base);   // lead * pace_blocks
  const long long span = (long long)ep.n_iter * ep.pace_blocks;                              // < 2^29 (launch_env)
  if (num < -span || num > span) return 0u;
  const int over_q8 = (int)((num * (long long)ep.pace_inv_q32) >> 24) - ep.pace_l0_q8;
  if (over_q8 <= 0) return 0u;
  t_own = min(t_own, 1u << 20);   // 10 ms: far beyond any iteration, keeps the product in range
  const unsigned long long d = ((unsigned long long)(unsigned)over_q8 * t_own) >> 8;
  return (unsigned)min(d, (unsigned long long)min(t_own >> 1, (unsigned)ep.pace_cap_ticks));
}

// One lane's count of an iteration start.  The per-lane opaque zero in the address keeps the compiler from rewriting the add as a
// wave reduction (its atomic optimizer does that to any add on a uniform address), whose result it would wait for on the spot:
// the returned value is meant to stay in flight behind the iteration's own loads.
__device__ __forceinline__ unsigned long long pace_count(const EnvParams& ep) {
  int z = 0;
  unsigned long long one = 1ull;
  asm volatile("" : "+v"(z), "+v"(one));   // (the increment too: as a loop invariant it would occupy two VGPRs for the whole launch)
  return __hip_atomic_fetch_add(ep.pace + z, one, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ void pace_sleep(unsigned ticks) {
  const unsigned long long t_in = wall_clock64();
  while (wall_clock64() - t_in < (unsigned long long)ticks) __builtin_amdgcn_s_sleep(16);
}

template <int TP, int TH, bool V = false>
__global__ __launch_bounds__(kEnvThreads) __attribute__((amdgpu_waves_per_eu(2, 2))) void env_rollout_kernel(EnvParams ep) {
  rollout_stagger(ep);
  unsigned long long pace_s = 0ull;
  unsigned pace_t0 = (unsigned)wall_clock64();
  const bool paced = ep.pace && ep.g_begin + (int)blockIdx.x * ep.gpw < ep.G;   // a workgroup without games does not count
#pragma clang loop unroll(disable)
  for (int iter = 0; iter < ep.n_iter; ++iter) {
    if (iter) __syncthreads();   // the previous iteration's rows have left LDS before they are cleared again
    if (paced) {
      // pacing (pace_delay): every point of this serial iteration is on the workgroup's critical path, so wave 0 sleeps right
      // here, on the lead its previous iteration start measured (that value has long arrived: the wait for it costs nothing
      // the first plane load below would not wait for anyway), and the other waves meet it at the body's first barrier
      const unsigned now = (unsigned)wall_clock64(), t_own = now - pace_t0;
      pace_t0 = now;
      if (threadIdx.x == 0) {
        if (iter > 0) {
          const unsigned d = pace_delay(ep, pace_s, iter - 1, t_own);
          if (d) pace_sleep(d);
        }
        pace_s = pace_count(ep);
      }
    }
    int zero = 0;
    asm volatile("" : "+s"(zero));
    env_body<3, TP, TH, V>(ep, nullptr, nullptr, zero, iter);
  }
}

// Wave-specialised, software-pipelined persistent rollout (128-thread workgroups, knowledge_mode 0).  Wave 0, the logic
// wave, runs the game logic of iteration k while wave 1, the stream wave, streams the rows of iteration k - 1 out of LDS and clears
// them (phase A); then both waves build the rows of k (phase B).  The logic wave issues no observation stores, so its waited loads
// (act counters, legal masks, mt19937 words) never queue behind a stream of kilobyte stores (vmcnt counts stores too); the stream
// wave issues no global loads.  HBM is written during the logic phase of every workgroup instead of only when the workgroups of a
// CU happen to be out of phase.  The state planes stay in LDS for the whole launch (loaded once, written back after the last
// iteration: nothing else reads them while the launch runs).  Same arithmetic, draw order and values as env_rollout_kernel: only
// which wave writes the rows, and when, differs.
// Which instances of env_rollout_pipe_kernel build their observation rows in registers (build_rows<.., FIXED>, hsad_obs_row.h):
// the fixed game shapes.  The generic instance has no compile-time offsets.  -DHSAD_ENV_ROWBUILD_SCATTER: none, for an A/B of the
// two builds within one tree.
#ifdef HSAD_ENV_ROWBUILD_SCATTER
template <int TP, int TH>
constexpr bool kRowBuildFixed = false;
#else
template <int TP, int TH>
constexpr bool kRowBuildFixed = TP > 0 && TH > 0;
#endif

__device__ __forceinline__ unsigned wave_sum(unsigned v) {
  for (int o = kWave / 2; o > 0; o >>= 1) v += (unsigned)__shfl_xor((int)v, o, kWave);
  return v;
}

// The chain of a call's launches (EnvParams::delta bits 1 and 2, EnvParams::phase; hsad_env_rollout_random).
// Launches 2, 3, ... of one call follow their predecessor on the same stream with nothing in between, so priv_s holds exactly the rows the predecessor's epilogue streamed.
// The predecessor leaves those bit rows in the workgroup's slice of the env's carry buffer and the follower takes them as the
// `prev` of its first stream, which then is a delta stream like every later one instead of 448 MB of lines HBM already holds.
// Blocks, g_begin and gpw are the same in every launch of a call: the slice index is the block index.
constexpr int kChainIn = 2, kChainOut = 4;   // in EnvParams::delta, next to bit 0 = the delta stream is on
constexpr int kPrioShift = 3;                // bits 3-4 of EnvParams::delta: the wave-priority mode (hsad_env_set_rollout_prio)
__device__ __forceinline__ uint4* chain_slice(const EnvParams& ep) {
  return reinterpret_cast<uint4*>(reinterpret_cast<uint32_t*>(ep.phase) + (size_t)blockIdx.x * ep.obs_words);
}

template <int TP, int TH>
__global__ __launch_bounds__(kEnvThreads) __attribute__((amdgpu_waves_per_eu(2, 2))) void env_rollout_pipe_kernel(EnvParams ep) {
  // The kernel is scheduled for two waves per SIMD (waves_per_eu(2, 2): four 128-thread workgroups per CU, which the LDS sizes,
  // delta_fits and the pacing assume), but the runtime places workgroups by the registers a kernel uses, not by that attribute.
  // With the rows built in registers the fixed instances use fewer than 171 VGPRs, the number from which a SIMD holds two waves
  // and not three; naming v175 keeps the allocation, and with it the residency and what configure_env_kernels decides from it,
  // where they were.  No instruction.
  if constexpr (kRowBuildFixed<TP, TH>) asm volatile("" ::: "v175");
  rollout_stagger(ep);
  extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
  uint32_t* s_st = smem;
  uint32_t* s_obs = s_st + ep.npl * kWave;
  uint32_t* s_legal = s_obs + ep.obs_words;
  uint32_t* s_own = s_legal + ep.legal_words;
  uint32_t* s_win = s_own + ep.own_words;
  uint32_t* s_grec = s_win + ep.win_words * kWave;
  float* s_eps = reinterpret_cast<float*>(s_grec + kWave);
  uint32_t* s_pace = s_grec + kWave + 128;   // one word: the delay (ticks) of the next stream, logic wave -> stream wave
  // ep.delta: a second copy of the observation bit rows behind everything else.  The rows of iteration i are built in copy i & 1;
  // while they are streamed the other copy still holds the rows of i - 1, which is what priv_s holds, so only the lines whose
  // word differs are stored.  The first stream of a launch stores every line: nothing is assumed about priv_s before the launch,
  // unless it is chained in (chain_slice above).
  // (the copy's address is worked out where it is used: as one more launch-long value it costs the generic instance a register it
  // does not have)
#define S_OBS1(z) (delta ? s_pace + 4 + (z) : s_obs)
  // bits 0-2 of ep.delta are the delta stream and its chain (kChainIn, kChainOut); bits 3-4 carry the wave-priority mode
  // (kPrioShift, hsad_env_set_rollout_prio), which is no business of the stream
  const int delta = ep.delta & 7;

  const int tid = threadIdx.x;
  const int lane = tid & (kWave - 1);
  const int wave = tid >> 6;
  const int g0 = ep.g_begin + blockIdx.x * ep.gpw;
  const int ng = min(ep.gpw, ep.G - g0);
  if (ng <= 0) return;
  const int P = TP ? TP : ep.P, H = TH ? TH : ep.H;

  // Wave priority (EnvParams::delta bits 3-4; hsad_env_set_rollout_prio).  Two waves share every SIMD for the whole launch, and
  // between equal priorities the older one wins the VALU arbitration every time.  Bit 0 (alternation): each wave takes priority
  // (iter ^ its hardware wave slot) & 1, so two co-tenants whose slots differ in bit 0 win in alternate iterations.  Bit 1 (role):
  // the stream wave, the iteration's critical chain, runs 2 above the logic wave.  Priority decides which wave issues first and
  // nothing else: no wave waits for another, and the results are the same in every mode.
  unsigned hw_self;
  asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw_self));
  const int prio_mode = (ep.delta >> kPrioShift) & 3;
  const int prio_role = (prio_mode & 2) ? 2 * __builtin_amdgcn_readfirstlane(wave) : 0;
  const int prio_alt = prio_mode & 1, prio_slot = (int)(hw_self & 15u);   // HW_ID [3:0]: the wave's slot on its SIMD

  // prologue: the logic wave stages the state planes and its act counters, the stream wave clears the rows and copies the eps list
  uint32_t act_counter = 0u;   // this lane's EnvParams::act_count, carried in a register for the launch (LogicCarry)
  uint64_t pkey[kPolicyKeys<TP, TH> ? 2 * TP : 1] = {};   // and its policy keys, where the instance has the registers
  if (wave == 0) {
    const int g = g0 + lane;
    if (lane < ng) {
      act_counter = ep.act_count[g];
      if constexpr (kPolicyKeys<TP, TH>) {
#pragma unroll
        for (int k = 0; k < 2 * TP; ++k) pkey[k] = policy_key(ep.policy_seed, (uint64_t)g, k >> 1, k & 1);
      }
      for (int p = 0; p < P; ++p) {   // the masks the previous launch, step or reset left: where build_rows leaves them from now on
        const uint64_t lm = ep.legal_bits[(size_t)g * P + p];
        s_win[(2 * p) * kWave + lane] = (uint32_t)lm;
        s_win[(2 * p + 1) * kWave + lane] = (uint32_t)(lm >> 32);
      }
    }
    for (int pl0 = 0; pl0 < ep.npl; pl0 += 8) {
      uint32_t v[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = ep.planes[(size_t)min(pl0 + j, ep.npl - 1) * ep.Gpad + g];
#pragma unroll
      for (int j = 0; j < 8; ++j)
        if (pl0 + j < ep.npl) ST(pl0 + j) = v[j];
    }
  } else {
    clear_rows(ep, s_obs, lane, kWave);
    if (delta & kChainIn) {   // the rows priv_s holds, into the copy the stream of iteration 1 compares against
      const uint4* src = chain_slice(ep);
      uint4* dst = reinterpret_cast<uint4*>(S_OBS1(0));
      for (int k = lane; k < (ep.obs_words >> 2); k += kWave) dst[k] = src[k];
    }
    for (int k = lane; k < min(ep.n_eps, 128); k += kWave) s_eps[k] = ep.eps_list[k];
    if (lane == 0) s_pace[0] = 0u;
    if (ep.dbg && ep.dbg_iters > 0 && lane == 0) s_pace[1] = hw_self;   // trace only: where the stream wave runs (STAMP_START_PIPE)
  }
  __syncthreads();

  unsigned pace_t0 = (unsigned)wall_clock64();
#pragma clang loop unroll(disable)
  for (int iter = 0; iter < ep.n_iter; ++iter) {
    int zero = 0;
    asm volatile("" : "+s"(zero));   // opaque zero: keeps the per-lane addresses inside the loop (see env_rollout_kernel)
    const int g = g0 + zero + lane;
    const bool valid = lane < ep.gpw && g < ep.G;
    const int dbg_it = iter;
    // one s_setprio per wave and iteration.  The instruction takes an immediate and ignores EXEC, so each form stands alone under
    // a condition formed through readfirstlane (scalar compare and branch, not an exec mask around an unconditional s_setprio).
    switch (__builtin_amdgcn_readfirstlane(prio_role + ((iter ^ prio_slot) & prio_alt))) {
      case 0: __builtin_amdgcn_s_setprio(0); break;
      case 1: __builtin_amdgcn_s_setprio(1); break;
      case 2: __builtin_amdgcn_s_setprio(2); break;
      default: __builtin_amdgcn_s_setprio(3); break;
    }
    STAMP_START_PIPE(s_pace[1]);
    // pacing: count this iteration start; the returned value is consumed in phase B, behind the logic's own waited loads
    unsigned long long pace_s = 0ull;
    if (ep.pace && tid == 0) pace_s = pace_count(ep);
    const unsigned pace_now = (unsigned)wall_clock64(), pace_t_own = pace_now - pace_t0;
    pace_t0 = pace_now;
    // ---- phase A: logic of iteration `iter` (wave 0) | rows of iteration `iter - 1` to HBM, then cleared (wave 1) ----
    Rng rng = {};
    float reward = 0.f;
    bool term = false;
    if (wave == 0) {
      if (ep.dbg && ep.dbg_iters > 0) {   // trace only: how long the previous iteration's stores keep wave 0's first load waiting
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        STAMP(1);
      }
      const uint32_t misc0 = ST(PL_MISC);
      const bool do_reset = valid && (!((misc0 >> 15) & 1u) || ((misc0 >> 14) & 1u));
      rng.mt = ep.mt + (size_t)g * kMtN;
      rng.draws = ST(PL_DRAWS);
      rng.la0 = ST(PL_LA0);
      rng.la1 = ST(PL_LA1);
      rng.la_n = (int)((misc0 >> 22) & 3u);
      rng.spos = (rng.draws + (uint32_t)rng.la_n) % (uint32_t)kMtN;
      uint32_t greedy_rec = 0;
      const LogicCarry carry = {&act_counter, s_win, pkey};
      env_logic<3, TP, TH, false, EnvParams, true>(ep, nullptr, nullptr, s_st, s_win, s_eps, lane, g, valid, do_reset, rng, greedy_rec, reward,
                                                   term, dbg_it, carry);
      s_grec[lane] = greedy_rec;
      STAMP(11);
    } else if (iter > 0) {
      if (ep.pace) {   // ahead of the mean: leave HBM to the others for a while (the logic wave waits at the barrier either way)
        const unsigned d = (unsigned)__builtin_amdgcn_readfirstlane((int)s_pace[0]);
        if (d) pace_sleep(d);
      }
      // rows of iter - 1; with delta, against the copy this iteration builds in, which holds the rows of iter - 2: the last ones
      // written (iter 1: nothing written yet, every line goes out, unless the launch is chained in: then that copy holds the rows
      // the launch before wrote last)
      uint32_t* s_obs1 = S_OBS1(zero);
      uint32_t* rows = (iter & 1) ? s_obs : s_obs1;
      uint32_t* prev = (iter & 1) ? s_obs1 : s_obs;
      const bool dbg_lines = ep.dbg && ep.dbg_iters > 0;
      int sl = lane;
      asm volatile("" : "+v"(sl));   // opaque: the stream's per-lane addresses are worked out here, not kept in registers for the launch
      unsigned units = 0;
      const bool all = !delta || (iter == 1 && !(delta & kChainIn));
      unsigned stored = stream_rows_delta(ep, rows, prev, all, s_legal, s_own, g0, ng, P, H, sl, kWave, dbg_lines, ep.compact, units);
      clear_words(prev, ep.obs_words, sl, kWave);
      clear_words(s_legal, ep.legal_words + ep.own_words, sl, kWave);
      if (dbg_lines) {
        stored = wave_sum(stored);
        if (lane == 0) env_stamp(ep, dbg_it, 13, stored);
        unsigned long long* dbg_units = reinterpret_cast<unsigned long long*>(((uint64_t)ep.dbg_units_hi << 32) | ep.dbg_units_lo);
        if (dbg_units) {
          units = wave_sum(units);
          if (lane == 0)
            dbg_units[((size_t)(ep.g_begin / ep.gpw) + blockIdx.x) * ep.dbg_iters + (size_t)min(dbg_it, ep.dbg_iters - 1)] = units;
        }
      }
      STAMP_T(8, kWave);
    }
    // the barrier's own wait, spelled out: LDS only.  (With the second form of the stream the compiler otherwise leaves an empty
    // s_waitcnt here; this one it keeps as it is.  It is the wait a barrier after LDS writes needs in any case.)
    __builtin_amdgcn_s_waitcnt(0xc07f);   // lgkmcnt(0)
    __syncthreads();
    STAMP(2);
    // ---- phase B: both waves build the rows of `iter`; wave 0 finishes the look-ahead refill and writes the scalars ----
    Refill rf;
    refill_issue(rf, rng, valid && wave == 0);
    if (valid)
      build_rows<TP, TH, false, kRowBuildFixed<TP, TH>>(ep, s_st, lane, g, (iter & 1) ? S_OBS1(zero) : s_obs, s_legal, s_own, s_grec[lane],
                                                        wave, 2, s_win);
    STAMP(3);
    if (valid && wave == 0) {
      refill_finish(rf, rng);
      ST(PL_DRAWS) = rng.draws;
      ST(PL_LA0) = rng.la0;
      ST(PL_LA1) = rng.la1;
      ST(PL_MISC) = (ST(PL_MISC) & ~(3u << 22)) | ((uint32_t)rng.la_n << 22);
      for (int p = 0; p < P; ++p) ep.eps[(size_t)g * P + p] = __uint_as_float(ST(PLEPS(p)));
      ep.reward[g] = reward;
      ep.terminal[g] = term ? 1 : 0;
      if (iter == ep.n_iter - 1) {
        for (int pl = 0; pl < ep.npl; ++pl) ep.planes[(size_t)pl * ep.Gpad + g] = ST(pl);
        ep.act_count[g] = act_counter;
      }
      if (ep.pace && lane == 0) {   // the delay of the stream of these rows (phase A of iter + 1), read after the barrier below
        const unsigned d = iter > 0 ? pace_delay(ep, pace_s, iter, pace_t_own) : 0u;
        s_pace[0] = d;
        if (ep.dbg && ep.dbg_iters > 0) env_stamp(ep, dbg_it, 12, d);
      }
    }
    __syncthreads();   // rows complete before wave 1 streams them; wave 1 done reading s_st before wave 0 changes it
    STAMP(4);
  }
  // epilogue: both waves stream the last iteration's rows, in the direct form (one stream of a launch: the compacted form's list
  // would have to be split between the waves for about 1 % of a 50-iteration launch)
  const int dbg_it = ep.n_iter - 1;
  {
    uint32_t* s_obs1 = S_OBS1(0);
    const uint32_t* rows = (ep.n_iter & 1) ? s_obs : s_obs1;
    uint32_t* prev = (ep.n_iter & 1) ? s_obs1 : s_obs;
    const bool dbg_lines = ep.dbg && ep.dbg_iters > 0;
    unsigned units = 0;
    unsigned stored = stream_rows_delta(ep, rows, prev, !delta || ep.n_iter == 1, s_legal, s_own, g0, ng, P, H, tid, ep.nthreads, dbg_lines,
                                        0, units);
    if (dbg_lines) {
      stored = wave_sum(stored);
      if (lane == 0) env_stamp(ep, dbg_it, 14 + wave, stored);
    }
    if (delta & kChainOut) {   // the rows just streamed, for the next launch of the call (the stream left them as they were)
      const uint4* src = reinterpret_cast<const uint4*>(rows);
      uint4* dst = chain_slice(ep);
      for (int k = tid; k < (ep.obs_words >> 2); k += ep.nthreads) dst[k] = src[k];
    }
  }
  STAMP(5);
#undef S_OBS1
}

// ---- init: zero planes, seed mt19937 (std::mt19937::seed: x0 = s; x_i = 1812433253*(x ^ x>>30) + i) ---
// game g's generator is seeded seed0 + (g % period); period <= 0: seed0 + g (hsad_env_create; hsad_env_reseed with no wrap)
__device__ __forceinline__ void init_game(const EnvParams& ep, int g, int seed0, int period) {
  if (g >= ep.Gpad) return;
  for (int pl = 0; pl < ep.npl; ++pl) ep.planes[(size_t)pl * ep.Gpad + g] = 0u;
  if (g >= ep.G) return;
  ep.planes[(size_t)PL_MISC * ep.Gpad + g] = 0u;  // not started, last_score = -1
  uint32_t* mt = ep.mt + (size_t)g * kMtN;
  uint32_t x = (uint32_t)(seed0 + (period > 0 ? g % period : g));
  mt[0] = x;
  for (int i = 1; i < kMtN; ++i) {
    x = 1812433253u * (x ^ (x >> 30)) + (uint32_t)i;
    mt[i] = x;
  }
  ep.act_count[g] = 0u;
}

__global__ void init_kernel(EnvParams ep) { init_game(ep, blockIdx.x * blockDim.x + threadIdx.x, ep.seed0, 0); }

__global__ void reseed_kernel(EnvParams ep, int seed0, int period) {
  init_game(ep, blockIdx.x * blockDim.x + threadIdx.x, seed0, period);
}

// ---- counter-based random-legal policy (kernel form; helpers are defined above env_kernel) ----
__global__ void policy_kernel(EnvParams ep, uint64_t seed, int64_t* __restrict__ a, int64_t* __restrict__ ga) {
  const int g = ep.g_begin + blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= ep.g_begin + ep.g_count || g >= ep.G) return;
  const uint32_t counter = ep.act_count[g];
  ep.act_count[g] = counter + 1u;
  for (int p = 0; p < ep.P; ++p) {
    const uint64_t mask = ep.legal_bits[(size_t)g * ep.P + p];  // same bits as the legal_move row
    a[(size_t)g * ep.P + p] = policy_pick(seed, (uint64_t)g, (uint64_t)counter, p, 0, mask);
    if (ga) ga[(size_t)g * ep.P + p] = policy_pick(seed, (uint64_t)g, (uint64_t)counter, p, 1, mask);
  }
}

// ---- getters ----------------------------------------------------------------------------------
#define GP(pl) ep.planes[(size_t)(pl) * ep.Gpad + g]

__global__ void query_kernel(EnvParams ep, int32_t* __restrict__ out) {
  const int g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= ep.G) return;
  const uint32_t board = GP(PL_BOARD), misc = GP(PL_MISC);
  int32_t* o = out + (size_t)g * HSAD_QUERY_WORDS;
  const bool started = misc_started(misc);
  o[HSAD_Q_TERMINATED] = misc_live(misc) ? 0 : 1;
  o[HSAD_Q_CUR_PLAYER] = board_cur(board);
  const int life = board_life(board);
  o[HSAD_Q_SCORE] = (life <= 0 && ep.bomb) ? 0 : board_fw_sum(board);
  o[HSAD_Q_LIFE] = life;
  o[HSAD_Q_INFO] = board_info(board);
  o[HSAD_Q_LAST_SCORE] = misc_last_score(misc);
  o[HSAD_Q_NUM_STEP] = misc_num_step(misc);
  o[HSAD_Q_DECK_SIZE] = misc_deck_size(misc);
  for (int c = 0; c < 5; ++c) o[HSAD_Q_FIREWORKS + c] = board_fw(board, c);
  o[HSAD_Q_RNG_DRAWS] = (int32_t)(GP(PL_DRAWS) & 0x7fffffffu);
  o[HSAD_Q_STARTED] = started ? 1 : 0;
  o[15] = 0;
}

__global__ void legal_query_kernel(EnvParams ep, const int32_t* __restrict__ uid, uint8_t* __restrict__ out) {
  const int g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= ep.G) return;
  const uint32_t board = GP(PL_BOARD);
  const int cur = board_cur(board);
  const MoveDec m = decode_uid(uid[g], ep.P, ep.H, RulesOf<true>::make(ep));
  bool ok = false;
  if (m.type != 0 && cur >= 0) {
    if (m.type <= 2) {
      const int len = (GP(PLH(cur)) >> 25) & 7;
      ok = (m.idx < len) && !(m.type == 2 && board_info(board) >= ep.max_info);
    } else if (board_info(board) > 0 && m.off >= 1 && m.off < ep.P) {
      int q = cur + m.off;
      if (q >= ep.P) q -= ep.P;
      ok = hand_match_mask(GP(PLH(q)), m.type == 3, m.val) != 0;
    }
  }
  out[g] = ok ? 1 : 0;
}

__global__ void deck_history_kernel(EnvParams ep, uint8_t* __restrict__ out, int32_t* __restrict__ count) {
  const int g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= ep.G) return;
  const uint32_t misc = GP(PL_MISC);
  const int n = misc_started(misc) ? ep.deck_max - misc_deck_size(misc) : 0;
  count[g] = ep.track_dh ? n : 0;
  for (int i = 0; i < 50; ++i) out[(size_t)g * 50 + i] = (ep.track_dh && i < n) ? ep.deck_hist[(size_t)g * 52 + i] : 0;
}

__global__ void export_state_kernel(EnvParams ep, int32_t* __restrict__ out, int words) {
  const int g = blockIdx.x * blockDim.x + threadIdx.x;
  const int P = ep.P;
  if (g >= ep.G) return;
  int32_t* o = out + (size_t)g * words;
  for (int i = 0; i < words; ++i) o[i] = 0;
  const uint64_t deck = (uint64_t)GP(PL_DECK_LO) | ((uint64_t)GP(PL_DECK_HI) << 32);
  const uint64_t disc = (uint64_t)GP(PL_DISC_LO) | ((uint64_t)GP(PL_DISC_HI) << 32);
  const uint32_t board = GP(PL_BOARD), misc = GP(PL_MISC), rec = GP(PL_LASTMV);
  for (int t = 0; t < 25; ++t) {
    o[t] = (int32_t)cnt2(deck, t);
    o[25 + t] = (int32_t)cnt2(disc, t);
  }
  for (int c = 0; c < 5; ++c) o[50 + c] = board_fw(board, c);
  o[55] = board_info(board);
  o[56] = board_life(board);
  o[57] = board_cur(board);
  o[58] = board_next(board);
  o[59] = board_turns(board);
  o[60] = misc_num_step(misc);
  o[61] = misc_deck_size(misc);
  const int type = rec & 7;
  o[62] = type;
  o[63] = -1;
  o[64] = o[65] = o[66] = o[67] = o[69] = o[70] = -1;
  if (type) {
    o[63] = (rec >> 3) & 7;
    if (type >= 3) {
      o[64] = (rec >> 6) & 7;
      if (type == 3) o[65] = (rec >> 9) & 7;
      if (type == 4) o[66] = (rec >> 12) & 7;
      o[68] = (rec >> 18) & 31;
    } else {
      o[67] = (rec >> 15) & 7;
      o[69] = (rec >> 23) & 7;
      o[70] = (rec >> 26) & 7;
      o[71] = (rec >> 29) & 1;
      o[72] = (rec >> 30) & 1;
    }
  }
  o[73] = (int32_t)(GP(PL_DRAWS) & 0x7fffffffu);
  o[74] = misc_last_score(misc);
  int base = 80;
  for (int p = 0; p < ep.P; ++p) {
    const uint32_t hw = GP(PLH(p)), kcp = GP(PLKCP(p)), krp = GP(PLKRP(p)), kh = GP(PLKH(p));
    const int len = (hw >> 25) & 7;
    for (int i = 0; i < ep.H; ++i) {
      int32_t* s = o + base + (p * ep.H + i) * 6;
      if (i < len) {
        s[0] = (hw >> (5 * i)) & 31;
        s[1] = (kcp >> (5 * i)) & 31;
        s[2] = (krp >> (5 * i)) & 31;
        s[3] = (int)((kh >> (6 * i)) & 7) - 1;
        s[4] = (int)((kh >> (6 * i + 3)) & 7) - 1;
      } else {
        s[0] = -1;
        s[3] = s[4] = -1;
      }
    }
  }
  base += ep.P * ep.H * 6;
  for (int p = 0; p < ep.P; ++p) {
    const uint32_t pw = misc_started(misc) ? GP(PLPERM(p)) : kIdentityPermBoth;
    for (int c = 0; c < 5; ++c) {
      o[base + p * 5 + c] = perm_c(pw & 0x7fffu, c);
      o[base + ep.P * 5 + p * 5 + c] = perm_c(pw >> 15, c);
    }
  }
}

// ---- host side ---------------------------------------------------------------------------------
thread_local std::string g_last_error;

int set_error(int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  g_last_error = buf;
  return code;
}

#define HIP_TRY(expr)                                                                              \
  do {                                                                                             \
    hipError_t e_ = (expr);                                                                        \
    if (e_ != hipSuccess) return set_error(HSAD_ERR_HIP, "%s failed: %s", #expr, hipGetErrorString(e_)); \
  } while (0)

}  // namespace

struct hsad_env {
  EnvParams ep;
  size_t lds_bytes;        // step kernel
  size_t lds_bytes_reset;  // reset kernel (adds the mt19937 prefetch window)
  size_t state_bytes;
  float* d_eps_list;
  bool bound;
  int device;
  // rollout partitions: independent game ranges on private streams so that one partition's
  // latency-bound phases overlap another partition's HBM-bound observation streaming
  long long stagger_ns;  // offset kept between consecutive partition chains (phase lock)
  unsigned long long* d_phase;     // [16][2] device words of the phase lock
  unsigned long long launch_seq;   // tag of the next locked launch
  int n_part;         // streams created so far
  int n_part_active;  // partitions used by hsad_env_rollout_random (1 = caller's stream only)
  int rollout_chunk;  // > 0: hsad_env_rollout_random runs persistent launches of this many iterations (hsad_env_set_rollout_chunk)
  int rollout_pipe;   // persistent launches use the pipelined schedule where it applies (developer switch HSAD_ENV_PIPE=0: the
                      // single-phase schedule of env_rollout_kernel everywhere, for A/B)
  // pacing of persistent launches (pace_delay).  Only paced launches touch the word, and each adds exactly pace_blocks x n_iter
  // to it, so the host knows its value at the start of the next one without a memset: *d_pace == pace_base between launches
  int rollout_pace;               // hsad_env_set_rollout_pace, HSAD_ENV_PACE at creation: 1 / 0; -1 neither (rollout_paced decides)
  // delta stream of the pipelined launches (EnvParams::delta).  Scope: one launch.  Nothing about priv_s is remembered between
  // launches, so reset / step / fork or a caller writing into priv_s cannot make anything stale.
  int rollout_delta;              // hsad_env_set_rollout_delta; HSAD_ENV_DELTA=0 at creation: every stream in full, for A/B
  int rollout_compact;            // hsad_env_set_rollout_compact; HSAD_ENV_COMPACT=0 at creation: the direct form of the delta stream
  int rollout_unit;               // hsad_env_set_rollout_unit; HSAD_ENV_UNIT=128|64 at creation: bytes of priv_s the compacted form
                                  // decides "changed" by (a line or a half line)
  bool delta_fits;                // the second copy of the rows costs the pipelined kernel no resident workgroup per CU
  size_t lds_bytes_delta;         // lds_bytes_reset + the second copy
  // chain of the delta launches of one hsad_env_rollout_random call (EnvParams::delta bits 1 and 2).  Scope: one call.  The first
  // launch of every call streams in full and never reads the buffer, so the rule above holds between calls as it did between
  // launches.
  int rollout_chain;              // hsad_env_set_rollout_chain; HSAD_ENV_CHAIN=0 at creation: every launch on its own, for A/B
  int rollout_prio;               // hsad_env_set_rollout_prio; HSAD_ENV_PRIO=0..3 at creation: wave priority in the pipelined kernel
                                  // (bit 0 alternation, bit 1 role; EnvParams::delta bits 3-4)
  uint32_t* d_chain;              // [workgroups][obs_words], allocated on first use
  bool chain_unavailable;         // that allocation failed: the env runs unchained
  unsigned long long* d_pace;     // the progress word (allocated with the env, zero)
  unsigned long long pace_base;   // its value once everything launched so far has run
  long long pace_bias;            // hsad_env_debug_pace_bias: added to the base the kernels are told, never to pace_base
  int pace_l0_q8, pace_cap_ticks; // dead band and delay cap (developer switches HSAD_ENV_PACE_L0_Q8 / HSAD_ENV_PACE_CAP_US)
  hipStream_t part_stream[16];
  hipEvent_t part_done[16];
  hipEvent_t part_begin[16];   // timing-enabled pair with part_done: per-partition chain time of the last rollout
  int last_rollout_iters, last_rollout_parts;
  hipEvent_t fork;
  int32_t* d_sel;     // [Gpad] which games hsad_env_determinize resampled (hsad_env_search.inc); allocated on first use
  // deal script (hsad_env_rewind_scripted).  scripted: hsad_env_step launches env_step_scripted_kernel; set by the first rewind,
  // cleared by hsad_env_reset / hsad_env_reseed.  The buffers are allocated on first use
  bool scripted;
  DealScript script;
  unsigned long long* d_sad;   // [Gpad * P] the SAD sections hsad_env_restore hands to the observe pass (hsad_env_position.inc); allocated on first use
  // replay of game records (hsad_env_record.inc), allocated on first use: the records of the last call, the script rows and counts
  // taken from them, and the action rows [2][Gpad * P] the replay steps on
  uint8_t* d_records;
  size_t d_records_cap;
  uint8_t* d_log_script;
  int32_t* d_log_count;
  int64_t* d_log_a;
};

namespace {

typedef void (*EnvKernelFn)(EnvParams, const int64_t*, const int64_t*);

// compile-time (players, hand) specialisations; anything else runs the generic <0,0> instance.  Variants (any rules but the
// full game's) run the generic instance with the rules read from EnvParams.
EnvKernelFn pick_env_kernel(int mode, int P, int H, bool variant) {
  if (variant) {
    switch (mode) {
      case 0: return env_kernel<0, 0, 0, true>;
      case 1: return env_kernel<1, 0, 0, true>;
      case 2: return env_kernel<2, 0, 0, true>;
      default: return env_kernel<3, 0, 0, true>;
    }
  }
#define HSAD_ENV_SPECIALISE(PP, HH)                 \
  if (P == PP && H == HH) {                         \
    switch (mode) {                                 \
      case 0: return env_kernel<0, PP, HH>;         \
      case 1: return env_kernel<1, PP, HH>;         \
      case 2: return env_kernel<2, PP, HH>;         \
      default: return env_kernel<3, PP, HH>;        \
    }                                               \
  }
  HSAD_ENV_SPECIALISE(2, 5)   // BASELINE configs[1..3]
  HSAD_ENV_SPECIALISE(5, 4)   // BASELINE configs[4] (5-player Other-Play)
  HSAD_ENV_SPECIALISE(3, 5)
  HSAD_ENV_SPECIALISE(4, 4)
#undef HSAD_ENV_SPECIALISE
  switch (mode) {
    case 0: return env_kernel<0, 0, 0>;
    case 1: return env_kernel<1, 0, 0>;
    case 2: return env_kernel<2, 0, 0>;
    default: return env_kernel<3, 0, 0>;
  }
}

// the step of an env that holds a deal script: the same (players, hand) choices as the plain step
typedef void (*EnvScriptedStepFn)(ScriptedParams, const int64_t*, const int64_t*);
EnvScriptedStepFn pick_scripted_step_kernel(int P, int H, bool variant) {
  if (variant) return env_step_scripted_kernel<0, 0, true>;
  if (P == 2 && H == 5) return env_step_scripted_kernel<2, 5>;
  if (P == 5 && H == 4) return env_step_scripted_kernel<5, 4>;
  if (P == 3 && H == 5) return env_step_scripted_kernel<3, 5>;
  if (P == 4 && H == 4) return env_step_scripted_kernel<4, 4>;
  return env_step_scripted_kernel<0, 0>;
}

typedef void (*EnvRolloutFn)(EnvParams);
// wave priority of the pipelined kernel (env_rollout_pipe_kernel, kPrioShift): the mode an env starts with.  2 = role: every SIMD
// holds the logic wave of one workgroup and the stream wave of another, and with the stream wave on top no workgroup's rate
// depends on which of the two arrived first (profiles/r18_env_prio_trace.json; headline profiles/r18_env_prio_ab.json)
constexpr int kRolloutPrioDefault = 2;
// pacing defaults (pace_delay): no dead band beyond the one the lead's definition brings (a workgroup in step with the others reads
// a lead of (-1, 0], so 0 already is half an iteration), one delay at most 35 us and never more than half the workgroup's own last
// iteration.  Measured against dead bands of 0.25 / 0.5 and caps of 20 / 60 us: profiles/r08_env_pace_ab.json
constexpr int kPaceL0Q8 = 0;
constexpr int kPaceCapTicks = 3500;
// the pipelined schedule (env_rollout_pipe_kernel) needs exactly one stream wave and no V0-belief fix-up of the streamed rows;
// 256-thread workgroups (few games per GPU), knowledge_mode 1 and variants run env_rollout_kernel
bool rollout_pipelined(const hsad_env* e) {
  return e->rollout_pipe && e->ep.nthreads == 2 * kWave && e->ep.kmode == 0 && !e->ep.variant;
}

// the delta stream needs the pipelined schedule, a float32 observation to skip lines of, and room for the second copy of the rows
bool rollout_delta_active(const hsad_env* e) {
  return e->rollout_delta && e->delta_fits && rollout_pipelined(e) && e->ep.obs_f32;
}

// Pacing is on unless switched off, except where the pipelined kernel runs the compacted delta stream: pacing was made for a
// write-bound iteration, in which a workgroup ahead of the mean only adds to the queue in front of HBM.  With the compacted
// stream the iteration is the chain stream -> build -> stream of a workgroup's own waves, and the sleep sits inside it
// (measured unpaced: -2.4 % at unit 128, -3.9 % at unit 64, profiles/r15_env_subline_ab.json; profiles/r16_env_rowbuild_ab.json).
bool rollout_paced(const hsad_env* e) {
  if (e->rollout_pace >= 0) return e->rollout_pace != 0;
  return !(e->rollout_compact && rollout_delta_active(e));
}

// the chain links launches that run the delta stream
int rollout_chain_mode(const hsad_env* e) {
  return rollout_delta_active(e) && !e->chain_unavailable ? e->rollout_chain : 0;
}

EnvRolloutFn pick_rollout_kernel(int P, int H, bool pipe, bool variant) {
  if (variant) return env_rollout_kernel<0, 0, true>;
#define HSAD_ROLLOUT_SPECIALISE(PP, HH) \
  if (P == PP && H == HH) return pipe ? env_rollout_pipe_kernel<PP, HH> : env_rollout_kernel<PP, HH>;
  HSAD_ROLLOUT_SPECIALISE(2, 5)
  HSAD_ROLLOUT_SPECIALISE(5, 4)
  HSAD_ROLLOUT_SPECIALISE(3, 5)
  HSAD_ROLLOUT_SPECIALISE(4, 4)
#undef HSAD_ROLLOUT_SPECIALISE
  return pipe ? env_rollout_pipe_kernel<0, 0> : env_rollout_kernel<0, 0>;
}

int configure_env_kernels(hsad_env* e) {
  HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(pick_rollout_kernel(e->ep.P, e->ep.H, false, e->ep.variant != 0)),
                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)e->lds_bytes_reset));
  // the pipelined kernel with and without the second copy of the observation rows: the delta stream is used only where the copy
  // leaves as many workgroups resident per CU as the kernel has without it (configs[1]: four)
  e->delta_fits = false;
  if (!e->ep.variant) {
    const void* fn = reinterpret_cast<const void*>(pick_rollout_kernel(e->ep.P, e->ep.H, true, false));
    const bool room = e->lds_bytes_delta <= 160 * 1024;
    HIP_TRY(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(room ? e->lds_bytes_delta : e->lds_bytes_reset)));
    if (room) {
      int wg_full = 0, wg_delta = 0;
      HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&wg_full, fn, 2 * kWave, e->lds_bytes_reset));
      HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&wg_delta, fn, 2 * kWave, e->lds_bytes_delta));
      e->delta_fits = wg_delta >= 1 && wg_delta >= wg_full;
    }
  }
  for (int mode = 0; mode < 4; ++mode) {
    const size_t lds = (mode == 1 || mode == 2) ? e->lds_bytes : e->lds_bytes_reset;
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(pick_env_kernel(mode, e->ep.P, e->ep.H, e->ep.variant != 0)),
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  }
  return HSAD_OK;
}

// launch one env kernel over games [g_begin, g_begin + g_count) (g_begin multiple of 64)
void launch_env(hsad_env* e, int mode, const int64_t* a, const int64_t* g, hipStream_t stream, int g_begin,
                int g_count, uint64_t policy_seed = 0, int64_t* a_out = nullptr, int64_t* g_out = nullptr, int part = -1,
                unsigned long long tag = 0, unsigned long long first_tag = 0, int n_part = 1, int n_iter = 1,
                int chain = 0) {
  size_t lds = (mode == 1 || mode == 2) ? e->lds_bytes : e->lds_bytes_reset;
  EnvParams ep = e->ep;
  ep.delta = mode == 3 && n_iter > 1 && rollout_delta_active(e) ? 1 : 0;
  ep.compact = ep.delta && e->rollout_compact ? (e->rollout_unit == 64 ? 2 : 1) : 0;
  if (ep.delta) lds = e->lds_bytes_delta;
  ep.phase = part >= 0 ? e->d_phase : nullptr;
  ep.part = part < 0 ? 0 : part;
  ep.lock_ticks = (int)(e->stagger_ns / 10);
  ep.launch_tag = tag;
  ep.first_tag = first_tag;
  if (part < 0 && ep.delta && chain && e->d_chain) {   // (EnvParams::delta: the chain of a call's persistent launches)
    ep.phase = reinterpret_cast<unsigned long long*>(e->d_chain);
    ep.delta |= chain;
  }
  // the wave-priority mode rides above the chain bits; only env_rollout_pipe_kernel looks at EnvParams::delta
  if (mode == 3 && n_iter > 1 && rollout_pipelined(e)) ep.delta |= e->rollout_prio << kPrioShift;
  ep.n_part = n_part;
  ep.g_begin = g_begin;
  ep.g_count = g_count;
  ep.policy_seed = policy_seed;
  ep.n_iter = n_iter;
  ep.stagger_ticks = n_iter > 1 ? (int)(e->stagger_ns / 10) : 0;
  static const int stagger_mode = getenv("HSAD_ENV_STAGGER_MODE") ? atoi(getenv("HSAD_ENV_STAGGER_MODE")) : 0;
  ep.stagger_mode = stagger_mode;
  ep.a_out = a_out;
  ep.g_out = g_out;
  ep.pace = nullptr;
  if (mode == 3 && n_iter > 1 && rollout_paced(e)) {
    // workgroups with games: the padded game count may add an empty one (32-game workgroups), which returns at once
    const int g_end = std::min(ep.G, g_begin + g_count);
    const long long blocks = g_end > g_begin ? (g_end - g_begin + ep.gpw - 1) / ep.gpw : 0;
    if (blocks > 0 && blocks * n_iter < (1ll << 29)) {   // pace_delay's fixed point
      ep.pace = e->d_pace;
      ep.pace_base = e->pace_base + (unsigned long long)e->pace_bias;
      ep.pace_blocks = (int)blocks;
      ep.pace_inv_q32 = (1ull << 32) / (unsigned long long)blocks;
      ep.pace_l0_q8 = e->pace_l0_q8;
      ep.pace_cap_ticks = e->pace_cap_ticks;
      e->pace_base += (unsigned long long)(blocks * n_iter);
    }
  }
  if (mode == 3 && n_iter > 1)
    hipLaunchKernelGGL(pick_rollout_kernel(ep.P, ep.H, rollout_pipelined(e), ep.variant != 0), dim3((g_count + ep.gpw - 1) / ep.gpw), dim3(ep.nthreads), lds, stream, ep);
  else if (mode == 1 && e->scripted) {
    ScriptedParams sp;
    static_cast<EnvParams&>(sp) = ep;
    sp.sc = e->script;
    hipLaunchKernelGGL(pick_scripted_step_kernel(ep.P, ep.H, ep.variant != 0), dim3((g_count + ep.gpw - 1) / ep.gpw), dim3(ep.nthreads),
                       lds, stream, sp, a, g);
  }
  else
    hipLaunchKernelGGL(pick_env_kernel(mode, ep.P, ep.H, ep.variant != 0), dim3((g_count + ep.gpw - 1) / ep.gpw), dim3(ep.nthreads), lds,
                       stream, ep, a, g);
}

}  // namespace

extern "C" {

const char* hsad_last_error(void) { return g_last_error.c_str(); }
// shared by the other translation units of libhsad (not part of the public header)
int hsad_internal_set_error(int code, const char* msg) {
  g_last_error = msg ? msg : "";
  return code;
}
const char* hsad_version(void) { return "hsad 0.1 gfx950"; }

int hsad_env_create(const hsad_env_config* cfg, hsad_env** out) { return hsad_env_create_rules(cfg, nullptr, out); }

int hsad_env_create_rules(const hsad_env_config* cfg, const hsad_env_rules* rules, hsad_env** out) {
  if (!cfg || !out) return set_error(HSAD_ERR_INVALID, "null argument");
  *out = nullptr;
  const hsad_env_rules full = {5, 5, 8, 3};
  const hsad_env_rules ru = rules ? *rules : full;
  if (ru.colors < 1 || ru.colors > 5) return set_error(HSAD_ERR_INVALID, "colors must be 1..5");
  if (ru.ranks < 1 || ru.ranks > 5) return set_error(HSAD_ERR_INVALID, "ranks must be 1..5");
  if (ru.max_information_tokens < 1 || ru.max_information_tokens > 8)
    return set_error(HSAD_ERR_INVALID, "max_information_tokens must be 1..8");
  if (ru.max_life_tokens < 1 || ru.max_life_tokens > 3) return set_error(HSAD_ERR_INVALID, "max_life_tokens must be 1..3");
  const int Cn = ru.colors, Rn = ru.ranks;
  const int deck_max = Cn * (Rn == 1 ? 3 : 2 * Rn);   // C * (3 + 2 (R - 2) + 1)
  if (cfg->num_games < 1) return set_error(HSAD_ERR_INVALID, "num_games must be >= 1");
  if (cfg->players < 2 || cfg->players > 5) return set_error(HSAD_ERR_INVALID, "players must be 2..5");
  if (cfg->hand_size < 1 || cfg->hand_size > 5) return set_error(HSAD_ERR_INVALID, "hand_size must be 1..5");
  if (cfg->players * cfg->hand_size > deck_max)
    return set_error(HSAD_ERR_INVALID, "players * hand_size (%d) exceeds the deck (%d cards)", cfg->players * cfg->hand_size, deck_max);
  if (cfg->shuffle_obs) return set_error(HSAD_ERR_INVALID, "shuffle_obs is not supported (reference asserts it off)");
  if (cfg->n_eps < 1 || !cfg->eps_list) return set_error(HSAD_ERR_INVALID, "eps_list must hold >= 1 value");
  if (cfg->knowledge_mode != 0 && cfg->knowledge_mode != 1) return set_error(HSAD_ERR_INVALID, "knowledge_mode 0|1");
  if (cfg->max_len > 255) return set_error(HSAD_ERR_INVALID, "max_len must be <= 255");
  if (cfg->games_per_workgroup != 0 && cfg->games_per_workgroup != 32 && cfg->games_per_workgroup != 64)
    return set_error(HSAD_ERR_INVALID, "games_per_workgroup must be 0 (auto), 32 or 64");
  HIP_TRY(hipSetDevice(cfg->device));

  hsad_env* e = new (std::nothrow) hsad_env();
  if (!e) return set_error(HSAD_ERR_NOMEM, "host allocation failed");
  std::memset(&e->ep, 0, sizeof(e->ep));
  EnvParams& ep = e->ep;
  ep.obs_f32 = 1;
  const int P = cfg->players, H = cfg->hand_size;
  ep.G = cfg->num_games;
  ep.Gpad = (ep.G + kWave - 1) / kWave * kWave;
  ep.P = P;
  ep.H = H;
  ep.nC = Cn;
  ep.nR = Rn;
  ep.max_info = ru.max_information_tokens;
  ep.max_life = ru.max_life_tokens;
  ep.deck_max = deck_max;
  ep.deck_full = deck_bits(Cn, Rn);
  ep.variant = (Cn != 5 || Rn != 5 || ep.max_info != 8 || ep.max_life != 3) ? 1 : 0;
  // canonical encoder sections: hands | board | discards | last action | card knowledge (| SAD's last action)
  ep.A = 2 * H + (P - 1) * (Cn + Rn) + 1;
  ep.DECKW = deck_max - P * H;
  ep.LAL = P + 4 + P + Cn + Rn + H + H + Cn * Rn + 2;
  ep.OB = P * H * Cn * Rn + P;
  ep.OD = ep.OB + ep.DECKW + Cn * Rn + ep.max_info + ep.max_life;
  ep.OL = ep.OD + deck_max;
  ep.OK = ep.OL + ep.LAL;
  ep.F0 = ep.OK + P * H * (Cn * Rn + Cn + Rn);
  ep.F = ep.F0 + (cfg->sad ? ep.LAL : 0);
  ep.max_len = cfg->max_len;
  ep.sad = cfg->sad ? 1 : 0;
  ep.shuffle_color = cfg->shuffle_color ? 1 : 0;
  ep.bomb = cfg->bomb ? 1 : 0;
  ep.kmode = cfg->knowledge_mode;
  ep.n_eps = cfg->n_eps;
  ep.track_dh = cfg->track_deck_history ? 1 : 0;
  ep.npl = PL_FIXED + 6 * P;
  ep.seed0 = cfg->seed0;
  ep.deal_mode = cfg->deal_mode ? 1 : 0;
  ep.nt_stores = getenv("HSAD_NT_STORES") ? atoi(getenv("HSAD_NT_STORES")) : 1;  // write-once obs stream: bypass L2 residency  // 1 = always take the literal fp64 discrete_distribution path
  {
    const int shuffle_draws = Cn == 1 ? 0 : (Cn % 2 == 0 ? 1 : 0) + (Cn - 1) / 2;   // std::shuffle of C colours
    const int n_static = 2 * P * H + P + (ep.shuffle_color ? 1 + shuffle_draws * (P - 1) : 0);
    ep.win_w = n_static + 2 < 64 ? n_static + 2 : 64;
    ep.win_words = ep.win_w <= 32 ? ep.win_w : 2 * ep.win_w + 1;
  }
  // +3 words of slack: or_bits may touch up to two words past the last row
  {
    // 32-game workgroups when 64-game ones would not even give every CU two (the persistent / fused kernels overlap one
    // workgroup's game logic with another's observation stream): 2-player games up to 32,768 per GPU, and the 5-player
    // configurations, whose 64-game bit rows need 60 KB of LDS
    int dev_cus = 256;
    (void)hipDeviceGetAttribute(&dev_cus, hipDeviceAttributeMultiprocessorCount, cfg->device);
    const int forced = getenv("HSAD_ENV_GPW") ? atoi(getenv("HSAD_ENV_GPW")) : cfg->games_per_workgroup;
    ep.gpw = (forced == 32 || forced == 64) ? forced : ((ep.G + kWave - 1) / kWave < 2 * dev_cus ? 32 : 64);
    // workgroup size: with two workgroups per CU or fewer, 128-thread workgroups leave a CU with four waves to clear, build and
    // stream its rows (5-player configs at 16,384 games: 52 % of the HBM roofline) -- give those launches four waves each
    const int forced_t = getenv("HSAD_ENV_THREADS") ? atoi(getenv("HSAD_ENV_THREADS")) : 0;
    const int n_wg = (ep.G + ep.gpw - 1) / ep.gpw;
    ep.nthreads = (forced_t == 128 || forced_t == 256) ? forced_t : (n_wg <= 2 * dev_cus ? 256 : 128);
  }
  ep.obs_words = (ep.gpw * P * ep.F + 31) / 32 + 3;
  ep.legal_words = (ep.gpw * P * ep.A + 31) / 32 + 3;
  ep.own_words = (ep.gpw * P * 3 * H + 31) / 32 + 3;
  ep.obs_words = (ep.obs_words + 3) & ~3;
  ep.legal_words = (ep.legal_words + 3) & ~3;
  ep.own_words = (ep.own_words + 3) & ~3;
  // + 4: the pacing word of the pipelined rollout behind the eps copy (kept a multiple of 16 bytes)
  e->lds_bytes = sizeof(uint32_t) * ((size_t)ep.npl * kWave + ep.obs_words + ep.legal_words + ep.own_words + kWave + 128 + 4);
  e->lds_bytes_reset = e->lds_bytes + sizeof(uint32_t) * (size_t)ep.win_words * kWave;
  e->lds_bytes_delta = e->lds_bytes_reset + sizeof(uint32_t) * (size_t)ep.obs_words;
  e->device = cfg->device;
  e->bound = false;
  e->n_part = 0;
  e->stagger_ns = 0;
  e->d_phase = nullptr;
  e->launch_seq = 0;
  e->last_rollout_iters = 0;
  e->last_rollout_parts = 0;
  e->n_part_active = 1;
  e->rollout_chunk = 0;
  e->rollout_pipe = getenv("HSAD_ENV_PIPE") ? atoi(getenv("HSAD_ENV_PIPE")) != 0 : 1;
  e->rollout_pace = getenv("HSAD_ENV_PACE") ? atoi(getenv("HSAD_ENV_PACE")) != 0 : -1;
  e->rollout_delta = getenv("HSAD_ENV_DELTA") ? atoi(getenv("HSAD_ENV_DELTA")) != 0 : 1;
  e->rollout_compact = getenv("HSAD_ENV_COMPACT") ? atoi(getenv("HSAD_ENV_COMPACT")) != 0 : 1;
  e->rollout_unit = getenv("HSAD_ENV_UNIT") && atoi(getenv("HSAD_ENV_UNIT")) == 128 ? 128 : 64;
  e->delta_fits = false;
  e->rollout_chain = getenv("HSAD_ENV_CHAIN") ? (atoi(getenv("HSAD_ENV_CHAIN")) != 0 ? 1 : 0) : 1;
  e->rollout_prio = getenv("HSAD_ENV_PRIO") ? atoi(getenv("HSAD_ENV_PRIO")) & 3 : kRolloutPrioDefault;
  e->d_chain = nullptr;
  e->chain_unavailable = false;
  e->d_pace = nullptr;
  e->pace_base = 0;
  e->pace_bias = 0;
  e->pace_l0_q8 = getenv("HSAD_ENV_PACE_L0_Q8") ? std::max(0, atoi(getenv("HSAD_ENV_PACE_L0_Q8"))) : kPaceL0Q8;
  e->pace_cap_ticks = getenv("HSAD_ENV_PACE_CAP_US") ? std::min(1000, std::max(0, atoi(getenv("HSAD_ENV_PACE_CAP_US")))) * 100 : kPaceCapTicks;
  e->fork = nullptr;
  e->d_sel = nullptr;
  e->scripted = false;
  e->script = DealScript{nullptr, nullptr};
  e->d_sad = nullptr;
  e->d_records = nullptr;
  e->d_records_cap = 0;
  e->d_log_script = nullptr;
  e->d_log_count = nullptr;
  e->d_log_a = nullptr;
  if (e->lds_bytes_reset > 160 * 1024) {
    const size_t need = e->lds_bytes_reset;
    delete e;
    return set_error(HSAD_ERR_INVALID, "configuration needs %zu B of LDS per wave (> 160 KiB)", need);
  }

  // + 64: with 32-game workgroups the idle lanes 32-63 of the last workgroup still LOAD their plane words
  const size_t planes_b = sizeof(uint32_t) * ((size_t)ep.npl * ep.Gpad + 64);
  const size_t mt_b = sizeof(uint32_t) * (size_t)ep.Gpad * kMtN;
  const size_t dh_b = (size_t)ep.Gpad * 52;
  hipError_t he;
  auto fail = [&](const char* what) {
    set_error(HSAD_ERR_NOMEM, "hipMalloc(%s) failed: %s", what, hipGetErrorString(he));
    hsad_env_destroy(e);
    return (int)HSAD_ERR_NOMEM;
  };
  if ((he = hipMalloc(&ep.planes, planes_b)) != hipSuccess) return fail("planes");
  if ((he = hipMalloc(&ep.mt, mt_b)) != hipSuccess) return fail("mt19937 state");
  if ((he = hipMalloc(&ep.deck_hist, dh_b)) != hipSuccess) return fail("deck history");
  if ((he = hipMalloc(&ep.err, 16)) != hipSuccess) return fail("error log");
  if ((he = hipMalloc(&ep.act_count, sizeof(uint32_t) * (ep.Gpad + 64))) != hipSuccess) return fail("act counters");
  if ((he = hipMalloc(&ep.legal_bits, sizeof(uint64_t) * (size_t)(ep.Gpad + 64) * P)) != hipSuccess) return fail("legal bits");
  HIP_TRY(hipMemset(ep.legal_bits, 0, sizeof(uint64_t) * (size_t)(ep.Gpad + 64) * P));
  if ((he = hipMalloc(&e->d_eps_list, sizeof(float) * cfg->n_eps)) != hipSuccess) return fail("eps list");
  if ((he = hipMalloc((void**)&e->d_pace, sizeof(unsigned long long))) != hipSuccess) return fail("pace word");
  HIP_TRY(hipMemset(e->d_pace, 0, sizeof(unsigned long long)));
  ep.eps_list = e->d_eps_list;
  e->state_bytes = planes_b + mt_b + dh_b;
  HIP_TRY(hipMemcpy(e->d_eps_list, cfg->eps_list, sizeof(float) * cfg->n_eps, hipMemcpyHostToDevice));
  HIP_TRY(hipMemset(ep.err, 0, 16));
  HIP_TRY(hipMemset(ep.deck_hist, 0, dh_b));
  {
    int rc = configure_env_kernels(e);
    if (rc != HSAD_OK) {
      hsad_env_destroy(e);
      return rc;
    }
  }
  hipLaunchKernelGGL(init_kernel, dim3((ep.Gpad + 255) / 256), dim3(256), 0, 0, ep);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipDeviceSynchronize());
  *out = e;
  return HSAD_OK;
}

void hsad_env_destroy(hsad_env* e) {
  if (!e) return;
  (void)hipSetDevice(e->device);
  if (e->d_phase) (void)hipFree(e->d_phase);
  if (e->d_pace) (void)hipFree(e->d_pace);
  if (e->d_chain) (void)hipFree(e->d_chain);
  if (e->d_sel) (void)hipFree(e->d_sel);
  if (e->script.cards) (void)hipFree(e->script.cards);
  if (e->script.count) (void)hipFree(e->script.count);
  if (e->d_sad) (void)hipFree(e->d_sad);
  if (e->d_records) (void)hipFree(e->d_records);
  if (e->d_log_script) (void)hipFree(e->d_log_script);
  if (e->d_log_count) (void)hipFree(e->d_log_count);
  if (e->d_log_a) (void)hipFree(e->d_log_a);
  if (e->ep.planes) (void)hipFree(e->ep.planes);
  if (e->ep.mt) (void)hipFree(e->ep.mt);
  if (e->ep.deck_hist) (void)hipFree(e->ep.deck_hist);
  if (e->ep.err) (void)hipFree(e->ep.err);
  if (e->ep.act_count) (void)hipFree(e->ep.act_count);
  if (e->ep.legal_bits) (void)hipFree(e->ep.legal_bits);
  if (e->d_eps_list) (void)hipFree(e->d_eps_list);
  for (int k = 0; k < e->n_part; ++k) {
    (void)hipStreamDestroy(e->part_stream[k]);
    (void)hipEventDestroy(e->part_done[k]);
    (void)hipEventDestroy(e->part_begin[k]);
  }
  if (e->fork) (void)hipEventDestroy(e->fork);
  delete e;
}

int hsad_env_feature_size(const hsad_env* e) { return e ? e->ep.F : 0; }
int hsad_env_num_action(const hsad_env* e) { return e ? e->ep.A : 0; }
int hsad_env_hand_feature_size(const hsad_env* e) { return e ? e->ep.H * e->ep.nC * e->ep.nR : 0; }
int hsad_env_get_rules(const hsad_env* e, hsad_env_rules* out) {
  if (!e || !out) return set_error(HSAD_ERR_INVALID, "null argument");
  out->colors = e->ep.nC;
  out->ranks = e->ep.nR;
  out->max_information_tokens = e->ep.max_info;
  out->max_life_tokens = e->ep.max_life;
  return HSAD_OK;
}
int hsad_env_max_deck_size(const hsad_env* e) { return e ? e->ep.deck_max : 0; }
int hsad_env_num_games(const hsad_env* e) { return e ? e->ep.G : 0; }
int hsad_env_num_players(const hsad_env* e) { return e ? e->ep.P : 0; }
int hsad_env_games_per_workgroup(const hsad_env* e) { return e ? e->ep.gpw : 0; }
int hsad_env_threads_per_workgroup(const hsad_env* e) { return e ? e->ep.nthreads : 0; }
int hsad_env_set_threads_per_workgroup(hsad_env* e, int threads) {
  if (!e || (threads != 128 && threads != 256)) return set_error(HSAD_ERR_INVALID, "threads per workgroup must be 128 or 256");
  e->ep.nthreads = threads;
  return HSAD_OK;
}
int64_t hsad_env_state_bytes(const hsad_env* e) { return e ? (int64_t)e->state_bytes : 0; }
int hsad_env_state_words(const hsad_env* e) { return e ? 80 + e->ep.P * e->ep.H * 6 + e->ep.P * 10 : 0; }

int hsad_env_bind_outputs(hsad_env* e, float* priv_s, float* legal_move, float* own_hand, float* eps, float* reward,
                          uint8_t* terminal) {
  if (!e) return set_error(HSAD_ERR_INVALID, "null env");
  if (!priv_s || !legal_move || !own_hand || !eps || !reward || !terminal)
    return set_error(HSAD_ERR_INVALID, "all six output tensors are required");
  if (((uintptr_t)priv_s & 15u) || ((uintptr_t)legal_move & 15u) || ((uintptr_t)own_hand & 15u))
    return set_error(HSAD_ERR_INVALID, "priv_s / legal_move / own_hand must be 16-byte aligned");
  e->ep.priv_s = priv_s;
  e->ep.legal = legal_move;
  e->ep.own = own_hand;
  e->ep.eps = eps;
  e->ep.reward = reward;
  e->ep.terminal = terminal;
  e->bound = true;
  return HSAD_OK;
}

int hsad_env_bind_packed(hsad_env* e, uint64_t* priv_bits, uint64_t* legal_bits, uint64_t* own_bits, void* priv_s_bf16,
                         int bf16_row_len, int keep_float32_obs) {
  if (!e) return set_error(HSAD_ERR_INVALID, "null env");
  if (e->ep.kmode != 0)
    return set_error(HSAD_ERR_INVALID, "the V0-belief observation (knowledge_mode 1) holds count ratios, not bits: no packed outputs");
  if (priv_s_bf16 && (bf16_row_len < e->ep.F || (bf16_row_len & 7) || ((uintptr_t)priv_s_bf16 & 15u)))
    return set_error(HSAD_ERR_INVALID, "bf16 rows must be 16-byte aligned and a multiple of 8 values >= feature_size long");
  if (!keep_float32_obs && !priv_bits && !priv_s_bf16)
    return set_error(HSAD_ERR_INVALID, "dropping the float32 observation needs at least one packed observation output");
  e->ep.priv_bits = reinterpret_cast<unsigned long long*>(priv_bits);
  e->ep.legal_out = reinterpret_cast<unsigned long long*>(legal_bits);
  e->ep.own_bits = reinterpret_cast<unsigned long long*>(own_bits);
  e->ep.priv16 = static_cast<unsigned short*>(priv_s_bf16);
  e->ep.pw64 = (e->ep.F + 63) / 64;
  e->ep.ld16 = bf16_row_len;
  e->ep.obs_f32 = keep_float32_obs ? 1 : 0;
  return HSAD_OK;
}

int hsad_env_reset(hsad_env* e, void* stream) {
  if (!e) return set_error(HSAD_ERR_INVALID, "null env");
  if (!e->bound) return set_error(HSAD_ERR_STATE, "hsad_env_bind_outputs must be called first");
  e->scripted = false;   // every game deals from its generator again
  launch_env(e, 0, nullptr, nullptr, (hipStream_t)stream, 0, e->ep.Gpad);
  HIP_TRY(hipGetLastError());
  return HSAD_OK;
}

int hsad_env_reseed(hsad_env* e, int32_t seed0, int32_t period, void* stream) {
  if (!e) return set_error(HSAD_ERR_INVALID, "null env");
  e->ep.seed0 = seed0;
  e->scripted = false;
  hipLaunchKernelGGL(reseed_kernel, dim3((e->ep.Gpad + 255) / 256), dim3(256), 0, (hipStream_t)stream, e->ep, (int)seed0, (int)period);
  HIP_TRY(hipGetLastError());
  return HSAD_OK;
}

// shared with csrc/hsad_eval.hip (not part of the public header): the plane of per-game status words the seat kernels read --
// started [15] | term [14] | last_score + 1 [16..21] -- and the sizes that go with it
int hsad_internal_env_status(const hsad_env* e, const uint32_t** misc, int* G, int* P, int* A, int* perfect_score) {
  if (!e) return set_error(HSAD_ERR_INVALID, "null env");
  *misc = e->ep.planes + (size_t)PL_MISC * e->ep.Gpad;
  *G = e->ep.G;
  *P = e->ep.P;
  *A = e->ep.A;
  *perfect_score = e->ep.nC * e->ep.nR;
  return HSAD_OK;
}

int hsad_env_step(hsad_env* e, const int64_t* a, const int64_t* greedy_a, void* stream) {
  if (!e) return set_error(HSAD_ERR_INVALID, "null env");
  if (!e->bound) return set_error(HSAD_ERR_STATE, "hsad_env_bind_outputs must be called first");
  if (!a) return set_error(HSAD_ERR_INVALID, "action tensor is null");
  if (e->ep.sad && !greedy_a) return set_error(HSAD_ERR_INVALID, "sad=1 requires greedy_a");
  launch_env(e, 1, a, greedy_a, (hipStream_t)stream, 0, e->ep.Gpad);
  HIP_TRY(hipGetLastError());
  return HSAD_OK;
}

int hsad_env_policy_random(hsad_env* e, uint64_t policy_seed, int64_t* a, int64_t* greedy_a, void* stream) {
  if (!e) return set_error(HSAD_ERR_INVALID, "null env");
  if (!e->bound) return set_error(HSAD_ERR_STATE, "hsad_env_bind_outputs must be called first");
  if (!a) return set_error(HSAD_ERR_INVALID, "action tensor is null");
  EnvParams ep = e->ep;
  ep.g_begin = 0;
  ep.g_count = ep.G;
  hipLaunchKernelGGL(policy_kernel, dim3((ep.G + 255) / 256), dim3(256), 0, (hipStream_t)stream, ep, policy_seed, a,
                     greedy_a);
  HIP_TRY(hipGetLastError());
  return HSAD_OK;
}

int hsad_env_set_partitions(hsad_env* e, int n_part) {
  if (!e) return set_error(HSAD_ERR_INVALID, "null env");
  if (n_part < 1 || n_part > 16) return set_error(HSAD_ERR_INVALID, "n_part must be 1..16");
  const int blocks = e->ep.Gpad / e->ep.gpw;
  if (n_part > blocks) n_part = blocks;
  HIP_TRY(hipSetDevice(e->device));
  for (int k = e->n_part; k < n_part; ++k) {
    HIP_TRY(hipStreamCreateWithFlags(&e->part_stream[k], hipStreamNonBlocking));
    HIP_TRY(hipEventCreate(&e->part_done[k]));
    HIP_TRY(hipEventCreate(&e->part_begin[k]));
  }
  if (!e->fork) HIP_TRY(hipEventCreateWithFlags(&e->fork, hipEventDisableTiming));
  if (n_part > e->n_part) e->n_part = n_part;
  e->n_part_active = n_part;
  return HSAD_OK;
}

int hsad_env_rollout_random(hsad_env* e, int n_iter, uint64_t policy_seed, int64_t* a, int64_t* greedy_a,
                            void* stream) {
  if (!e) return set_error(HSAD_ERR_INVALID, "null env");
  if (!e->bound) return set_error(HSAD_ERR_STATE, "hsad_env_bind_outputs must be called first");
  if (!a) return set_error(HSAD_ERR_INVALID, "action tensor is null");
  if (e->ep.sad && !greedy_a) return set_error(HSAD_ERR_INVALID, "sad=1 requires greedy_a");
  if (e->scripted) return set_error(HSAD_ERR_STATE, "hsad_env_rollout_random: the env holds a deal script (only hsad_env_step deals from it; hsad_env_reset clears it)");
  const int K = e->n_part_active;
  const int blocks = e->ep.Gpad / e->ep.gpw;
  if (e->rollout_chunk > 0) {   // persistent: one launch = rollout_chunk iterations of every game (the last one may be shorter)
    // The chain: a launch hands its last rows to the next one of this call where both run the delta stream (more than one
    // iteration each).  The launches follow each other on one stream, so nothing can touch priv_s in between; the first launch
    // of the call is never chained in, whatever an earlier call left in the buffer.
    bool chained = rollout_chain_mode(e) != 0 && n_iter > e->rollout_chunk;
    if (chained && !e->d_chain) {
      if (hipMalloc((void**)&e->d_chain, sizeof(uint32_t) * (size_t)blocks * e->ep.obs_words) != hipSuccess) {
        (void)hipGetLastError();   // no room: not an error, the env runs unchained from now on
        e->d_chain = nullptr;
        e->chain_unavailable = true;
        chained = false;
      }
    }
    int chain = 0;
    for (int i = 0; i < n_iter; i += e->rollout_chunk) {
      const int n = std::min(e->rollout_chunk, n_iter - i), n_next = std::min(e->rollout_chunk, n_iter - i - n);
      chain = (chain & kChainOut ? kChainIn : 0) | (chained && n > 1 && n_next > 1 ? kChainOut : 0);
      launch_env(e, 3, nullptr, nullptr, (hipStream_t)stream, 0, e->ep.Gpad, policy_seed, a, greedy_a, -1, 0, 0, 1, n, chain);
    }
    HIP_TRY(hipGetLastError());
    return HSAD_OK;
  }
  if (K <= 1) {
    for (int i = 0; i < n_iter; ++i)
      launch_env(e, 3, nullptr, nullptr, (hipStream_t)stream, 0, e->ep.Gpad, policy_seed, a, greedy_a);
    HIP_TRY(hipGetLastError());
    return HSAD_OK;
  }
  // fork: every partition stream waits for the work already queued on the caller's stream
  HIP_TRY(hipEventRecord(e->fork, (hipStream_t)stream));
  for (int k = 0; k < K; ++k) {
    HIP_TRY(hipStreamWaitEvent(e->part_stream[k], e->fork, 0));
    HIP_TRY(hipEventRecord(e->part_begin[k], e->part_stream[k]));
  }
  e->last_rollout_iters = n_iter;
  e->last_rollout_parts = K;
  // the chains are phase-locked in the kernel (EnvParams::phase): partition k starts each launch stagger_ns after
  // partition k-1 started the launch of the same iteration
  if (!e->d_phase) {
    HIP_TRY(hipMalloc((void**)&e->d_phase, sizeof(unsigned long long) * 32));
    HIP_TRY(hipMemset(e->d_phase, 0, sizeof(unsigned long long) * 32));
  }
  const unsigned long long first_tag = e->launch_seq + 1;
  for (int i = 0; i < n_iter; ++i) {
    const unsigned long long tag = ++e->launch_seq;
    for (int k = 0; k < K; ++k) {
      const int b0 = (int)((long long)blocks * k / K), b1 = (int)((long long)blocks * (k + 1) / K);
      if (b1 <= b0) continue;
      launch_env(e, 3, nullptr, nullptr, e->part_stream[k], b0 * e->ep.gpw, (b1 - b0) * e->ep.gpw, policy_seed, a, greedy_a, k, tag,
                 first_tag, K);
    }
  }
  HIP_TRY(hipGetLastError());
  // join
  for (int k = 0; k < K; ++k) {
    HIP_TRY(hipEventRecord(e->part_done[k], e->part_stream[k]));
    HIP_TRY(hipStreamWaitEvent((hipStream_t)stream, e->part_done[k], 0));
  }
  return HSAD_OK;
}

int hsad_env_last_rollout_ms(hsad_env* e, float* ms_per_launch, int* n_part) {
  if (!e || !ms_per_launch) return set_error(HSAD_ERR_INVALID, "null argument");
  const int K = e->last_rollout_parts;
  if (n_part) *n_part = K;
  if (K < 2 || e->last_rollout_iters < 1) return set_error(HSAD_ERR_STATE, "no partitioned rollout has run");
  for (int k = 0; k < K; ++k) {
    float ms = 0.f;
    HIP_TRY(hipEventSynchronize(e->part_done[k]));
    HIP_TRY(hipEventElapsedTime(&ms, e->part_begin[k], e->part_done[k]));
    ms_per_launch[k] = ms / (float)e->last_rollout_iters;
  }
  return HSAD_OK;
}

int hsad_env_set_rollout_chunk(hsad_env* e, int iterations_per_launch) {
  if (!e || iterations_per_launch < 0) return set_error(HSAD_ERR_INVALID, "bad argument");
  e->rollout_chunk = iterations_per_launch;
  return HSAD_OK;
}

int hsad_env_set_rollout_pace(hsad_env* e, int on) {
  if (!e) return set_error(HSAD_ERR_INVALID, "null env");
  e->rollout_pace = on != 0;
  return HSAD_OK;
}

int hsad_env_rollout_pace_cap_us(const hsad_env* e) { return e ? e->pace_cap_ticks / 100 : 0; }

int hsad_env_set_rollout_delta(hsad_env* e, int on) {
  if (!e) return set_error(HSAD_ERR_INVALID, "null env");
  e->rollout_delta = on != 0;
  return HSAD_OK;
}

int hsad_env_rollout_delta_active(const hsad_env* e) { return e && rollout_delta_active(e) ? 1 : 0; }

int hsad_env_set_rollout_chain(hsad_env* e, int mode) {
  if (!e || (mode != 0 && mode != 1)) return set_error(HSAD_ERR_INVALID, "the rollout chain mode is 0 or 1");
  e->rollout_chain = mode;
  return HSAD_OK;
}

int hsad_env_rollout_chain_active(const hsad_env* e) { return e ? rollout_chain_mode(e) : 0; }

int hsad_env_set_rollout_prio(hsad_env* e, int mode) {
  if (!e || mode < 0 || mode > 3) return set_error(HSAD_ERR_INVALID, "the rollout priority mode is 0..3");
  e->rollout_prio = mode;
  return HSAD_OK;
}

int hsad_env_rollout_prio(const hsad_env* e) { return e && rollout_pipelined(e) ? e->rollout_prio : 0; }

int hsad_env_set_rollout_compact(hsad_env* e, int on) {
  if (!e) return set_error(HSAD_ERR_INVALID, "null env");
  e->rollout_compact = on != 0;
  return HSAD_OK;
}

int hsad_env_rollout_compact_active(const hsad_env* e) { return e && e->rollout_compact && rollout_delta_active(e) ? 1 : 0; }

int hsad_env_set_rollout_unit(hsad_env* e, int bytes) {
  if (!e || (bytes != 128 && bytes != 64)) return set_error(HSAD_ERR_INVALID, "the rollout unit is 128 or 64 bytes");
  e->rollout_unit = bytes;
  return HSAD_OK;
}

int hsad_env_rollout_unit(const hsad_env* e) { return e ? (hsad_env_rollout_compact_active(e) ? e->rollout_unit : 128) : 0; }

int hsad_env_debug_pace_bias(hsad_env* e, int64_t bias) {
  if (!e) return set_error(HSAD_ERR_INVALID, "null env");
  e->pace_bias = (long long)bias;
  return HSAD_OK;
}

int hsad_env_debug_pace_word(hsad_env* e, int64_t* device_word, int64_t* host_base) {
  if (!e || !device_word || !host_base) return set_error(HSAD_ERR_INVALID, "null argument");
  unsigned long long w = 0;
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(&w, e->d_pace, sizeof(w), hipMemcpyDeviceToHost));
  *device_word = (int64_t)w;
  *host_base = (int64_t)e->pace_base;
  return HSAD_OK;
}

int hsad_env_set_rollout_stagger(hsad_env* e, int microseconds) {
  if (!e || microseconds < 0) return set_error(HSAD_ERR_INVALID, "bad argument");
  e->stagger_ns = (long long)microseconds * 1000;
  return HSAD_OK;
}

int hsad_env_query(hsad_env* e, int32_t* out, void* stream) {
  if (!e || !out) return set_error(HSAD_ERR_INVALID, "null argument");
  hipLaunchKernelGGL(query_kernel, dim3((e->ep.G + 255) / 256), dim3(256), 0, (hipStream_t)stream, e->ep, out);
  HIP_TRY(hipGetLastError());
  return HSAD_OK;
}

int hsad_env_move_is_legal(hsad_env* e, const int32_t* uid, uint8_t* out, void* stream) {
  if (!e || !uid || !out) return set_error(HSAD_ERR_INVALID, "null argument");
  hipLaunchKernelGGL(legal_query_kernel, dim3((e->ep.G + 255) / 256), dim3(256), 0, (hipStream_t)stream, e->ep, uid,
                     out);
  HIP_TRY(hipGetLastError());
  return HSAD_OK;
}

int hsad_env_deck_history(hsad_env* e, uint8_t* out, int32_t* count, void* stream) {
  if (!e || !out || !count) return set_error(HSAD_ERR_INVALID, "null argument");
  hipLaunchKernelGGL(deck_history_kernel, dim3((e->ep.G + 255) / 256), dim3(256), 0, (hipStream_t)stream, e->ep, out,
                     count);
  HIP_TRY(hipGetLastError());
  return HSAD_OK;
}

int hsad_env_export_state(hsad_env* e, int32_t* out, void* stream) {
  if (!e || !out) return set_error(HSAD_ERR_INVALID, "null argument");
  hipLaunchKernelGGL(export_state_kernel, dim3((e->ep.G + 255) / 256), dim3(256), 0, (hipStream_t)stream, e->ep, out,
                     hsad_env_state_words(e));
  HIP_TRY(hipGetLastError());
  return HSAD_OK;
}

int hsad_env_debug_timing(hsad_env* e, uint64_t* buf) {
  if (!e) return set_error(HSAD_ERR_INVALID, "null env");
  e->ep.dbg = reinterpret_cast<unsigned long long*>(buf);
  e->ep.dbg_iters = 0;
  return HSAD_OK;
}

int hsad_env_debug_trace(hsad_env* e, uint64_t* buf, int n_iters) {
  if (!e || (buf && n_iters < 1)) return set_error(HSAD_ERR_INVALID, "bad argument");
  e->ep.dbg = reinterpret_cast<unsigned long long*>(buf);
  e->ep.dbg_iters = buf ? n_iters : 0;
  return HSAD_OK;
}

int hsad_env_debug_units(hsad_env* e, uint64_t* buf) {
  if (!e) return set_error(HSAD_ERR_INVALID, "null env");
  e->ep.dbg_units_lo = (unsigned)(reinterpret_cast<uint64_t>(buf) & 0xffffffffull);
  e->ep.dbg_units_hi = (unsigned)(reinterpret_cast<uint64_t>(buf) >> 32);
  return HSAD_OK;
}

int64_t hsad_env_rollout_lds_bytes(const hsad_env* e) {
  return e ? (int64_t)(rollout_delta_active(e) ? e->lds_bytes_delta : e->lds_bytes_reset) : 0;
}

int hsad_env_rollout_resident_workgroups(const hsad_env* e) {
  if (!e) return 0;
  const void* fn = reinterpret_cast<const void*>(pick_rollout_kernel(e->ep.P, e->ep.H, rollout_pipelined(e), e->ep.variant != 0));
  int n = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, fn, e->ep.nthreads, (size_t)hsad_env_rollout_lds_bytes(e)) != hipSuccess) return -1;
  return n;
}

int hsad_env_error_count(hsad_env* e, int32_t* count, int32_t* first_game, int32_t* first_code) {
  if (!e || !count) return set_error(HSAD_ERR_INVALID, "null argument");
  uint32_t h[4] = {0, 0, 0, 0};
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(h, e->ep.err, 16, hipMemcpyDeviceToHost));
  *count = (int32_t)h[0];
  if (first_game) *first_game = (int32_t)h[1];
  if (first_code) *first_code = (int32_t)h[2];
  if (h[0]) HIP_TRY(hipMemset(e->ep.err, 0, 16));
  return HSAD_OK;
}

}  // extern "C"

// fork / determinise / observe / playout: the env as a simulator for test-time search
#include "hsad_env_search.inc"

// the exact belief over a hidden hand and the rejection-free sampler on top of it
#include "hsad_env_belief.inc"

// positions in and out: import of the canonical record, snapshot and restore of whole games
#include "hsad_env_position.inc"

// rule-list bots as a policy: one call on the planes, and whole playouts in one launch
#include "hsad_env_rulebot.inc"

// game records: replay a logged game to any move in one launch
#include "hsad_env_record.inc"
