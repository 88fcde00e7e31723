/* hsad.h — C ABI of libhsad.so, the MI355X-native hot path of facebookresearch/hanabi_SAD.
 *
 * This is the drop-in boundary: plain pointers, sizes and opaque handles only (no torch types).
 * Every entry point cites the reference interface it replaces (paths relative to the reference
 * tree).  Device pointers are HIP device addresses (e.g. torch.Tensor.data_ptr() of a ROCm
 * tensor); `stream` is a hipStream_t passed as void* (NULL = default stream).
 *
 * Conventions: functions return 0 on success and a negative hsad_status otherwise;
 * hsad_last_error() gives the message for the calling thread.  Nothing aborts the process —
 * where the reference assert(false)s (illegal move, stepping a finished game:
 * cpp/hanabi_env.cc:50,63-80) the kernels record the offending game in a device-side error log
 * that hsad_env_error_count() reads back, and leave that game untouched.
 */
#ifndef HSAD_H_
#define HSAD_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
  HSAD_OK = 0,
  HSAD_ERR_INVALID = -1, /* bad argument / configuration            */
  HSAD_ERR_HIP = -2,     /* a HIP runtime call failed               */
  HSAD_ERR_STATE = -3,   /* call sequence violates the API contract */
  HSAD_ERR_NOMEM = -4
} hsad_status;

const char* hsad_last_error(void);
/* library / build identification ("hsad <ver> gfx950") */
const char* hsad_version(void);

/* ------------------------------------------------------------------------------------------
 * Batched Hanabi environment: G concurrent games stepped by one HIP launch.
 * Replaces hanalearn.HanabiEnv / HanabiVecEnv (cpp/pybind.cc:14-43, cpp/hanabi_env.h:17-168,
 * rela/env.h:29-108) and the absent HLE engine + CanonicalObservationEncoder they call.
 * ------------------------------------------------------------------------------------------ */
typedef struct hsad_env hsad_env;

typedef struct hsad_env_config {
  int32_t num_games;      /* G >= 1 (one reference HanabiEnv object per game: create.py:36-53)      */
  int32_t players;        /* params["players"]   2..5                                               */
  int32_t hand_size;      /* params["hand_size"] 1..5                                               */
  int32_t bomb;           /* params["bomb"]: 1 => score 0 once all life tokens are lost             */
  int32_t seed0;          /* game g is seeded seed0 + g (create.py:41)                              */
  int32_t max_len;        /* HanabiEnv maxLen; <=0 disables forced truncation (hanabi_env.h:87-91)  */
  int32_t sad;            /* append greedy-action last-action section (hanabi_env.cc:82-91,154-160) */
  int32_t shuffle_obs;    /* must be 0 (selfplay.py:175 asserts it; 2-player hack in the reference) */
  int32_t shuffle_color;  /* Other-Play colour permutation (hanabi_env.cc:22-44,145-152,176-181)    */
  int32_t knowledge_mode; /* 0 = binary card-knowledge section, 1 = V0-belief weighted section      */
  int32_t n_eps;          /* length of eps_list (hanabi_env.cc:18-20)                               */
  int32_t device;         /* HIP device ordinal                                                     */
  int32_t track_deck_history; /* keep per-game dealt-card log for deck_history()                    */
  int32_t deal_mode;      /* 0 = exact integer fast path with fp64 fallback (default); 1 = always run the
                             literal libstdc++ discrete_distribution fp64 arithmetic (same results)   */
  int32_t games_per_workgroup; /* kernel shape: 64 or 32 games per workgroup, 0 = chosen from num_games and the
                             CU count (32 when 64-game workgroups would leave fewer than two per CU).  Scheduling
                             only -- results are identical; both shapes are parity-tested                  */
  const float* eps_list;  /* HOST pointer, n_eps floats                                             */
} hsad_env_config;

int hsad_env_create(const hsad_env_config* cfg, hsad_env** out);
void hsad_env_destroy(hsad_env* env);

/* The game's rules: HLE's `colors`, `ranks`, `max_information_tokens`, `max_life_tokens` (HanabiGame params, passed
 * whole by the reference: cpp/hanabi_env.h:27).  The full game is 5 / 5 / 8 / 3; each may be lowered to 1.  Card
 * instances per colour: 3 of rank 0, 1 of rank R-1, 2 of every other rank (R = 1: 3); deck = C * sum.  Every size
 * follows: A = 2H + (P-1)(C+R) + 1, F = P*H*C*R + P + (deck - P*H) + C*R + max_info + max_life + deck
 * + LAL + P*H*(C*R + C + R) with LAL = 2P + 4 + C + R + 2H + C*R + 2 (SAD: + LAL). */
typedef struct hsad_env_rules {
  int32_t colors;                  /* 1..5 */
  int32_t ranks;                   /* 1..5 */
  int32_t max_information_tokens;  /* 1..8 */
  int32_t max_life_tokens;         /* 1..3 */
} hsad_env_rules;

/* hsad_env_create with the game's rules; rules == NULL is the full game (exactly hsad_env_create).  Refuses values outside
 * the bounds above and a deal larger than the deck (players * hand_size > deck). */
int hsad_env_create_rules(const hsad_env_config* cfg, const hsad_env_rules* rules, hsad_env** out);
int hsad_env_get_rules(const hsad_env* env, hsad_env_rules* out);
/* HanabiGame::MaxDeckSize: 50 for the full game */
int hsad_env_max_deck_size(const hsad_env* env);

/* HanabiEnv::featureSize / numAction / handFeatureSize (cpp/hanabi_env.h:53-72) and batch dims. */
int hsad_env_feature_size(const hsad_env* env);
int hsad_env_num_action(const hsad_env* env);
int hsad_env_hand_feature_size(const hsad_env* env);
int hsad_env_num_games(const hsad_env* env);
int hsad_env_num_players(const hsad_env* env);
/* the kernel shape in use (32 or 64 games per workgroup; hsad_env_config.games_per_workgroup) */
int hsad_env_games_per_workgroup(const hsad_env* env);
/* workgroup size of the env kernels: 128 (one logic wave + one helper) or 256 (three helpers for clearing, building and streaming
 * the rows; chosen when the launch has at most two workgroups per CU).  Results never depend on it; the setter is for tests. */
int hsad_env_threads_per_workgroup(const hsad_env* env);
int hsad_env_set_threads_per_workgroup(hsad_env* env, int threads);
/* bytes of internal device state held by the env (state planes + per-game mt19937) */
int64_t hsad_env_state_bytes(const hsad_env* env);

/* Output tensors, owned by the caller, dense row-major, written by reset/step:
 *   priv_s     float32 [G, P, F]        legal_move float32 [G, P, A]
 *   own_hand   float32 [G, P, hand*3]   eps        float32 [G, P]
 *   reward     float32 [G]              terminal   uint8   [G]
 * = the TensorDict {"priv_s","legal_move","eps","own_hand"} + reward + terminal that
 * VectorEnv::reset/step stack over envs (rela/env.h:48-87; cpp/hanabi_env.cc:197-204).
 * priv_s must be 16-byte aligned. */
int hsad_env_bind_outputs(hsad_env* env, float* priv_s, float* legal_move, float* own_hand, float* eps,
                          float* reward, uint8_t* terminal);

/* Outputs for DEVICE consumers, written by reset/step next to (or instead of) the float32 tensors from the same on-chip bit rows:
 *   priv_bits  uint64 [G*P, ceil(F/64)]   the observation as bit words = the stored format of an HSAD_BITS field
 *                                         (hsad_seqwriter_set_prepacked: no pack pass, 1/32 of the bytes)
 *   legal_bits uint64 [G*P]               bit uid = legal_move[uid]          own_bits uint64 [G*P]   bit j = own_hand[j]
 *   priv_s_bf16 bf16  [G*P, row_len]      the first GEMM's operand, columns F.. zero (hsad_r2d2_act priv_s_bf16: no cast pass)
 * Any pointer may be NULL.  keep_float32_obs = 0 stops writing the float32 priv_s tensor (the reference's API-boundary format,
 * 3.3 KB per row) -- legal_move / own_hand / eps / reward / terminal are always written.  Not available with knowledge_mode 1. */
int hsad_env_bind_packed(hsad_env* env, uint64_t* priv_bits, uint64_t* legal_bits, uint64_t* own_bits, void* priv_s_bf16,
                         int bf16_row_len, int keep_float32_obs);

/* VectorEnv::reset (rela/env.h:48-60): (re)starts every game for which terminated() holds —
 * all of them on the first call — and rewrites only those games' observation rows
 * (HanabiEnv::reset, cpp/hanabi_env.cc:9-47). */
int hsad_env_reset(hsad_env* env, void* stream);

/* Puts every game back to "not started" (what hsad_env_create leaves) with game g's generator seeded seed0 + (g % period);
 * period <= 0 = no wrap (seed0 + g, the seeding of hsad_env_create).  A following hsad_env_reset starts all games.  Games with
 * equal seeds that receive equal actions stay bit-identical (eps draw, colour permutation, deck): groups of `period` games
 * replay the same deals, and one env object serves chunk after chunk of deals.  Launch-only. */
int hsad_env_reseed(hsad_env* env, int32_t seed0, int32_t period, void* stream);

/* VectorEnv::step (rela/env.h:66-87) / HanabiEnv::step (cpp/hanabi_env.cc:49-113).
 * a, greedy_a: device int64 [G, P] = reply["a"], reply["greedy_a"]; greedy_a may be NULL when sad=0. */
int hsad_env_step(hsad_env* env, const int64_t* a, const int64_t* greedy_a, void* stream);

/* Uniform-random-legal policy on the device (BASELINE.json configs[1]; stand-in for
 * R2D2Agent.act's multinomial branch, pyhanabi/r2d2.py:270).  Reads the env's compact legal-move
 * bit masks (the same bits the legal_move tensor is expanded from), writes a and greedy_a [G, P] int64 (noop for players not on turn) and advances the per-game
 * decision counter.  Stream: counter-based hash keyed (policy_seed, seed0-relative game id, counter). */
int hsad_env_policy_random(hsad_env* env, uint64_t policy_seed, int64_t* a, int64_t* greedy_a, void* stream);

/* n_iter iterations of the reference thread loop body (cpp/thread_loop.h:46-72) for all games:
 * reset-terminated -> random policy -> step, fused into ONE launch per iteration (the sampled a / greedy_a are
 * still written to the given tensors; trajectories are identical to hsad_env_reset + hsad_env_policy_random +
 * hsad_env_step).  Launch-only; returns before the GPU finishes. */
int hsad_env_rollout_random(hsad_env* env, int n_iter, uint64_t policy_seed, int64_t* a, int64_t* greedy_a,
                            void* stream);

/* Split the games into n_part (1..16) independent ranges that hsad_env_rollout_random runs on private
 * HIP streams (fork/join around the caller's stream), so one range's latency-bound reset/logic phases
 * overlap another range's HBM-bound observation streaming.  Results are unaffected (games are
 * independent).  Default 1 = everything on the caller's stream. */
int hsad_env_set_partitions(hsad_env* env, int n_part);

/* Persistent rollout: with iterations_per_launch > 0 hsad_env_rollout_random runs ONE launch per that many iterations
 * (the last may be shorter); inside it every workgroup advances its 64 games independently -- games never interact, so
 * nothing but the launch boundary ever synchronised them -- and workgroup b starts (b % 8) x the rollout stagger late so
 * that the workgroups of a CU stream their observations at different times.  Takes precedence over partitions; 0 (the
 * default) = one launch per iteration and partition.  Results are bit-identical either way. */
int hsad_env_set_rollout_chunk(hsad_env* env, int iterations_per_launch);
/* Pacing of persistent launches.  Default: on, except where the pipelined launches run the compacted delta stream
 * (hsad_env_rollout_compact_active), whose iteration is no longer write-bound and only loses the delay.  HSAD_ENV_PACE=0 / 1 when
 * the env is created, or a call here, decides for every kind of launch.  The
 * workgroups of a launch run at persistently different rates and the launch ends on the slowest.  Every workgroup counts its
 * iteration starts on one device word of the env; one that is ahead of the mean by more than a dead band delays its next
 * observation stream by (lead - dead band) x its own iteration time, at most hsad_env_rollout_pace_cap_us(), and so leaves HBM
 * bandwidth to the others.  No workgroup waits for another and no work moves: timing only, results are bit-identical. */
int hsad_env_set_rollout_pace(hsad_env* env, int on);
/* longest delay of one iteration, microseconds */
int hsad_env_rollout_pace_cap_us(const hsad_env* env);
/* Delta stream of the pipelined persistent launches (on by default; HSAD_ENV_DELTA=0 when the env is created, or on = 0 here, gives
 * the full stream, for A/B).  One move changes little of an observation, so within one launch every observation stream after the
 * first stores only the 128-byte lines of priv_s whose bits differ from what the stream before wrote; the workgroup keeps those bits
 * in a second copy of its LDS rows.  The first stream of every launch stores everything and nothing is carried between launches
 * (except between the launches of one call, which nothing can come between: hsad_env_set_rollout_chain below), so whatever happens
 * to priv_s or the games between calls cannot matter.  Results are bit-identical.  The packed outputs, legal
 * moves and own hand are streamed in full.  hsad_env_rollout_delta_active: whether persistent launches use it now -- not without the
 * pipelined schedule or the float32 observation, and not where the second copy would cost a resident workgroup per CU. */
int hsad_env_set_rollout_delta(hsad_env* env, int on);
int hsad_env_rollout_delta_active(const hsad_env* env);
/* Chain of the launches of one hsad_env_rollout_random call (mode 1, the default; HSAD_ENV_CHAIN=0 when the env is created, or mode 0
 * here, runs every launch on its own, for A/B).  A persistent call of more than one launch issues its launches back to back on one
 * stream, so launch 2, 3, ... finds in priv_s exactly the rows its predecessor streamed last.  The predecessor leaves those bit rows
 * in a buffer of the env ([workgroups][row words], allocated by the first call that needs it; if that fails the env runs unchained
 * and reports no error) and the follower's first stream stores only what changed against them, like every later stream of the
 * launch, instead of every line.  Only launches that run the delta stream are linked (a last launch of one iteration is not).
 * The first launch of every call stores everything and never reads the buffer: nothing is carried from one call to the next, so
 * reset, step, fork or a caller writing into priv_s between calls still cannot matter.  Results are bit-identical.
 * hsad_env_rollout_chain_active: the mode in use, 0 wherever hsad_env_rollout_delta_active is false. */
int hsad_env_set_rollout_chain(hsad_env* env, int mode);
int hsad_env_rollout_chain_active(const hsad_env* env);
/* Compacted form of the delta stream (on by default wherever the delta stream is active; HSAD_ENV_COMPACT=0 when the env is created,
 * or on = 0 here, gives the direct form, for A/B).  The stream wave first lists the lines that changed, in place in the LDS copy it
 * has just compared, and then stores from the list, eight whole lines per wave-store.  The same lines are stored either way: results
 * are bit-identical.  hsad_env_rollout_compact_active: true only where hsad_env_rollout_delta_active is. */
int hsad_env_set_rollout_compact(hsad_env* env, int on);
int hsad_env_rollout_compact_active(const hsad_env* env);
/* Unit of the compacted form: the bytes of priv_s it decides "changed" by.  128 is a whole line (one 32-bit word of the bit rows),
 * 64 a half line (16 bits), which is one native write request of the L2: a line whose change sits in one half then costs half the
 * bytes (-20 % of the bytes written at configs[1]).  Results are bit-identical either way, and units may change between launches.
 * HSAD_ENV_UNIT=128|64 when the env is created, or bytes here; the default is 64 (2-3 % faster at the median with the pacing on,
 * 4 % without; DESIGN.md 3a has the runs).  hsad_env_rollout_unit: the unit persistent launches use as the env stands, 128
 * wherever hsad_env_rollout_compact_active is false (the direct form and the epilogue stream always go by lines). */
int hsad_env_set_rollout_unit(hsad_env* env, int bytes);
int hsad_env_rollout_unit(const hsad_env* env);
/* Wave priority in the pipelined persistent kernel (HSAD_ENV_PRIO=0..3 when the env is created, or mode here; default 2).  Four workgroups
 * of two waves share a CU for the whole launch, two waves per SIMD, and between equal priorities the older wave wins the issue
 * arbitration every time.  Bit 0, alternation: at the top of every iteration a wave takes priority (iteration ^ its hardware
 * wave slot) & 1, so co-tenants whose slots differ in bit 0 win in turn.  Bit 1, role: the stream wave runs 2 above the logic
 * wave.  Priority only decides which wave issues first: no workgroup waits for another and results are bit-identical in every
 * mode.  hsad_env_rollout_prio: the mode persistent launches use as the env stands, 0 wherever the pipelined kernel does not
 * run (256-thread workgroups, knowledge_mode 1, variants).  DESIGN.md 3a has the measurements behind the default. */
int hsad_env_set_rollout_prio(hsad_env* env, int mode);
int hsad_env_rollout_prio(const hsad_env* env);
/* Test seams of the pacing.  bias is added to the counter base every later persistent launch is told (not to the host's own
 * record), so that every workgroup's lead reads bias / workgroups iterations too high: all far ahead (bias > 0) or far behind (bias < 0); 0
 * restores the truth.  A lead no launch could produce (beyond its iteration count) switches the delay off.
 * hsad_env_debug_pace_word synchronises the device and returns the progress word and the value the host expects it to hold. */
int hsad_env_debug_pace_bias(hsad_env* env, int64_t bias);
int hsad_env_debug_pace_word(hsad_env* env, int64_t* device_word, int64_t* host_base);
/* Phase lock of the partition chains of hsad_env_rollout_random: partition k starts each launch `microseconds` after
 * partition k-1 started the launch of the same iteration (bounded in-kernel wait on a device timestamp), so that one
 * partition's latency-bound logic phase keeps overlapping another's HBM stream.  Timing only -- results are identical
 * for any value; 0 lets the chains drift. */
int hsad_env_set_rollout_stagger(hsad_env* env, int microseconds);
/* average launch duration (ms) on each partition stream of the last partitioned hsad_env_rollout_random (HIP events on
 * the streams the kernels were launched on; synchronises those events); ms_per_launch [n_part <= 16] */
int hsad_env_last_rollout_ms(hsad_env* env, float* ms_per_launch, int* n_part);

/* Per-game scalars, device int32 [G, HSAD_QUERY_WORDS]:
 * terminated(), getCurrentPlayer(), getScore(), getLife(), getInfo(), lastScore(), numStep,
 * deck size, getFireworks()[5], rng draws consumed  (cpp/hanabi_env.h:81-135). */
#define HSAD_QUERY_WORDS 16
enum {
  HSAD_Q_TERMINATED = 0, HSAD_Q_CUR_PLAYER = 1, HSAD_Q_SCORE = 2, HSAD_Q_LIFE = 3, HSAD_Q_INFO = 4,
  HSAD_Q_LAST_SCORE = 5, HSAD_Q_NUM_STEP = 6, HSAD_Q_DECK_SIZE = 7, HSAD_Q_FIREWORKS = 8 /* ..12 */,
  HSAD_Q_RNG_DRAWS = 13, HSAD_Q_STARTED = 14
};
int hsad_env_query(hsad_env* env, int32_t* out, void* stream);

/* HanabiEnv::moveIsLegal (cpp/hanabi_env.h:103-106): uid device int32 [G] -> out device uint8 [G]. */
int hsad_env_move_is_legal(hsad_env* env, const int32_t* uid, uint8_t* out, void* stream);

/* HanabiEnv::deckHistory (cpp/hanabi_env.h:112-114): dealt cards of the current episode as
 * colour*5+rank bytes, out device uint8 [G, 50], count device int32 [G]. */
int hsad_env_deck_history(hsad_env* env, uint8_t* out, int32_t* count, void* stream);

/* Canonical int32 state dump [G, hsad_env_state_words()] for parity tests (layout documented in
 * oracle/hanabi_oracle.cc orc_env_export_state; the two sides are written independently). */
int hsad_env_state_words(const hsad_env* env);
int hsad_env_export_state(hsad_env* env, int32_t* out, void* stream);

/* Developer aid: when buf != NULL (device uint64 [ceil(G/64), 8]) the reset/step kernels store
 * s_memtime stamps at their phase boundaries (load, logic, build rows, write-back, stream). */
int hsad_env_debug_timing(hsad_env* env, uint64_t* buf);
/* Developer aid: per-iteration trace of a persistent rollout.  buf (device uint64 [Gpad / games_per_workgroup, n_iters, 16]) receives
 * wall_clock64 stamps (100 MHz) of every iteration plus each workgroup's HW_ID / XCC_ID; slot map in csrc/hsad_env.hip (env_stamp).
 * buf == NULL switches the trace (and hsad_env_debug_timing) off. */
int hsad_env_debug_trace(hsad_env* env, uint64_t* buf, int n_iters);
/* Developer aid, with hsad_env_debug_trace: buf (device uint64 [Gpad / games_per_workgroup, n_iters], the trace's n_iters) receives
 * the number of units of priv_s the stream wave stored for the rows of each iteration's predecessor, counted in the unit that stream
 * decided by: half lines where hsad_env_rollout_unit is 64 (the first stream of a launch, which stores everything, and the direct
 * form count lines).  Slot 13 of the trace keeps counting 128-byte lines with any change.  Written only while the trace is on;
 * buf == NULL switches it off. */
int hsad_env_debug_units(hsad_env* env, uint64_t* buf);
/* Dynamic LDS bytes per workgroup of the reset / rollout kernels (what a persistent rollout launch requests: with the second copy
 * of the observation rows while hsad_env_rollout_delta_active). */
int64_t hsad_env_rollout_lds_bytes(const hsad_env* env);
/* Workgroups of the persistent rollout kernel this env launches (pipelined or single-phase, its workgroup size, the LDS bytes
 * above) that one CU holds at a time: hipOccupancyMaxActiveBlocksPerMultiprocessor.  -1 if the query fails. */
int hsad_env_rollout_resident_workgroups(const hsad_env* env);

/* Number of games that hit an API-contract error (illegal move, step on a finished game) since
 * the last call; synchronises the device.  first_game/first_code (may be NULL) describe the first.
 * Codes: 1 illegal move, 2 illegal greedy move, 3 step on a finished game, 4 hsad_env_fork / hsad_env_restore source index out of
 * range, 5 a deal script names a card the deck does not hold (hsad_env_rewind_scripted), 6 hsad_env_import_state / hsad_env_restore
 * refused a position (the call's status word holds the HSAD_POS_* flags that say why), 7 a hsad_env_policy_rule seat_bot entry names
 * no bot, 8 hsad_env_playout_logged met a logged move that is illegal where the record makes it. */
int hsad_env_error_count(hsad_env* env, int32_t* count, int32_t* first_game, int32_t* first_code);

/* ---- The env as a simulator for test-time search (determinised Monte Carlo, SPARTA-style single-agent search): branch a game,
 * resample the hidden hand, play out.  The reference has no such call; nothing below changes what reset / step / rollout compute.
 *
 * hsad_env_fork: dst game j becomes a copy of src game src_index[j] (device int32 [G_dst]); -1 leaves game j untouched, any other
 * value outside [0, G_src) leaves it untouched too and is counted in dst's error log (code 4; nothing is read out of bounds).
 * Copied: every state plane (eps and colour permutation included), the policy counter, and the deck-history row when both envs
 * track it.  seeds == NULL copies the generator as well (its 624 words, the draw counter, the look-ahead): the fork then deals
 * exactly what the source will deal.  seeds = device int32 [G_dst] gives game j the generator std::mt19937(seeds[j]) with no draw
 * consumed.  A source game that is not started or is finished is copied as it is (a later hsad_env_reset restarts it).
 * Afterwards all bound outputs of the forked games are rewritten from the copied state ("observe": the rows of the last reset or
 * step of the source, bit for bit), reward = 0, terminal = the state's terminated bit; a game that was never started gets all-zero
 * rows.  Untouched games keep theirs.  The SAD greedy-action section is no function of the state: it is copied from src's
 * currently bound observation rows (bit words if bound, else float32), so a sad = 1 fork is refused when src has neither.
 * HSAD_ERR_INVALID when players, hand size, rules, sad, shuffle_color, knowledge_mode, bomb, max_len or the device differ, when
 * dst == src, or when dst tracks the deck history and src does not.  Launch-only; src is read on `stream`. */
int hsad_env_fork(hsad_env* dst, hsad_env* src, const int32_t* src_index, const int32_t* seeds, void* stream);

/* hsad_env_determinize: in place, resamples the hand of player viewer[g] (device int32 [G]; -1, or a game that is not started or
 * is finished: skipped) uniformly from the hands its card knowledge allows.  key (device int64 [G]) is the "game" field of the
 * counter-based hash, seed its seed: equal (seed, key) on equal states give equal worlds.  tries_out (device int32 [G] or NULL):
 * tries used, 0 if skipped, -1 if the sampler gave up after 32 tries and kept the hand.  Per game, card type t = colour * 5 + rank:
 *   pool[t] = deck count + copies in the viewer's hand;  compat_i[t] = colour(t) and rank(t) both plausible for slot i;
 *   Zmax_i = sum_t pool[t] compat_i[t];  for try = 0..31: q = pool; for slot i = 0..L-1: Z = sum_t q[t] compat_i[t] (0 fails the
 *   try), h = hash(seed, key, try * 8 + i, 64), k = (h * Z) >> 32, card = lowest t whose running sum of q compat_i exceeds k,
 *   q[card] -= 1;  u = hash(seed, key, try * 8 + 7, 64);  accept iff u * prod Zmax_i < (prod Z) << 32.
 * hash = the policy's (mix64-based) hash with stream 64.  On acceptance the hand holds the sampled cards in slot order and the deck
 * counts become q; deck size, knowledge, discards, board, last move and generator are unchanged.  The proposal has probability
 * prod q_i / Z_i and is kept with probability prod Z_i / Zmax_i, so accepted hands are proportional to the product of the falling
 * counts: uniform over the physical unseen cards consistent with the knowledge (multiply-shift bias < 2^-26).  The rows of the
 * resampled games are then rewritten by the observe pass (SAD section kept from the env's own rows).  Launch-only. */
int hsad_env_determinize(hsad_env* env, const int32_t* viewer, const int64_t* key, uint64_t seed, int32_t* tries_out, void* stream);

/* The exact belief over the viewer's hidden hand, and a sampler without rejection on top of it.  Notation as above: card type
 * t = colour * 5 + rank, pool[t] = deck count + copies in the viewer's hand, occupied slots i = 0 .. n-1 (n <= 5) in slot order,
 * compat_i[t] = colour(t) and rank(t) both plausible for slot i.  The belief is the distribution hsad_env_determinize samples:
 * uniform over the injective assignments of PHYSICAL unseen cards to the slots that agree with compat.  For a set of slots B let
 * s_B(q) = sum_t q[t] prod_{i in B} compat_i[t] (the cards plausible for every slot of B).  The number of assignments for slots S:
 *   C({}, q) = 1;   C(S, q) = sum over B subset of S with min(S) in B of (-1)^(|B|-1) (|B|-1)! s_B(q) C(S \ B, q)
 * (inclusion-exclusion over which slots were given the same card: Moebius inversion on the lattice of set partitions), exact in
 * int64 (every term < 2^35, N = C(all slots, pool) < 2^28).  Marginals: num[i][t] = pool[t] compat_i[t] C(all \ {i}, pool - e_t),
 * sum_t num[i][t] = N, P(slot i holds type t) = num[i][t] / N.  Unrank, r in [0, N), q = pool: for slot i = 0 .. n-1, for t
 * ascending with q[t] compat_i[t] != 0: c = C({i+1 .. n-1}, q - e_t), w = q[t] c; r < w: slot i holds t, q[t] -= 1, r = r mod c,
 * next slot; else r -= w.  Exactly prod of the falling counts ranks arrive at each hand: its weight in the belief.
 *
 * hsad_env_hand_belief: viewer device int32 [G]; a game with viewer -1 or out of range, never started or finished is skipped.
 * total_out device int64 [G] = N (0 if skipped); counts_out device int64 [G, H, 25] = num (empty slots and skipped games all zero);
 * trinary_out device int64 [G, H, 3] or NULL = num summed by the classes of EncodeOwnHandTrinary against the firework fw of the
 * card's colour: [rank == fw (playable), rank < fw, rank > fw].  Reads the state only: no bound output is needed or touched (it
 * works on a sad = 1 env with no observation rows).  Launch-only.
 *
 * hsad_env_determinize_exact: hsad_env_determinize's in-place counterpart with the same skip rules: the hand of viewer[g] becomes
 * unrank(r) in slot order, the deck counts the q it leaves; everything else in the state is unchanged.  rank_in device int64 [G]:
 * r = rank_in[g] (key, seed and stratum are ignored, key may be NULL).  rank_in NULL: the stratified rank of world w = stratum[g]
 * (device int32 [G], NULL = 0) of W = n_strata:
 *   lo = (w N) / W, hi = ((w + 1) N) / W, u = (hash(seed, key[g], 0, 65) << 32) | hash(seed, key[g], 1, 65),
 *   r = lo + ((u * (hi - lo)) >> 64)   (r = lo for an empty stratum)
 * with hash the policy's hash, stream 65 (hsad_env_determinize uses 64).  The W worlds of a game thus cover [0, N) evenly; W = 1 is
 * a plain exact draw.  There is no try count and no giving up.  A game is LEFT ALONE -- state and rows -- when it is skipped, when
 * rank_in[g] is outside [0, N), when stratum[g] is outside [0, W) or when N = 0 (a live game's true hand is consistent, so N >= 1).
 * rank_out device int64 [G] or NULL: the rank used, -1 for every game left alone.  The rows of the resampled games are rewritten by
 * the observe pass, SAD section kept from the env's own rows: the precondition and error of hsad_env_determinize with sad = 1.
 * HSAD_ERR_INVALID when n_strata < 1 or > 2^20.  Launch-only. */
int hsad_env_hand_belief(hsad_env* env, const int32_t* viewer, int64_t* total_out, int64_t* counts_out, int64_t* trinary_out, void* stream);
int hsad_env_determinize_exact(hsad_env* env, const int32_t* viewer, const int64_t* key, uint64_t seed, const int32_t* stratum, int n_strata,
                               const int64_t* rank_in, int64_t* rank_out, void* stream);

/* The learned hand belief on the env (model: hsad_belief_tail below; row: csrc/hsad_belief_head.h).
 * hsad_env_hand_knowledge: for every seat p of every game g, what hsad_env_hand_belief counts with for viewer p, and the seat's true
 * hand: pool_out device int64 [G, P] (deck count + copies in the seat's hand, two bits per card type), compat_out device int32
 * [G, P, H] (the 25-bit mask of the types plausible for the slot; 0 for an empty slot), cards_out device int32 [G, P, H] (the card
 * type, -1 for an empty slot).  A game that was never started or is finished gets zeros and -1.  Reads the state only.
 * hsad_env_determinize_belief: hsad_env_determinize_exact's counterpart that samples the hand of viewer[g] from the learned belief
 * under logits fp32 [G, ldz] (row g: 25 logits per slot, ldz >= 25 H): slot by slot with u_i = hash(seed, key[g], i, 66), the
 * policy's hash on stream 66, as hsad_belief_tail's model prescribes in sample mode.  Same skip rules, same LEFT ALONE semantics
 * (also for a row with a non-finite logit on an occupied slot), same observe pass afterwards and the same sad = 1 precondition.  The
 * deck counts become the pool the sample leaves.  status_out device int32 [G] or NULL: 1 sampled, 0 left alone; logp_out device
 * float [G] or NULL: the log-probability of the sampled hand under the belief (0 when left alone).  With all-zero logits the
 * distribution is hsad_env_determinize_exact's.  Every sampled hand is consistent with the card knowledge and the card counts.
 * Launch-only. */
int hsad_env_hand_knowledge(hsad_env* env, int64_t* pool_out, int32_t* compat_out, int32_t* cards_out, void* stream);
int hsad_env_determinize_belief(hsad_env* env, const int32_t* viewer, const float* logits, int ldz, const int64_t* key, uint64_t seed,
                                float* logp_out, int32_t* status_out, void* stream);

/* hsad_env_determinize_belief_worlds: hsad_env_determinize_belief for a search env, whose slots are forks of a few root games.  Env
 * game g reads logits row row[g] of fp32 [n_rows, ldz] (row device int32 [G]; NULL = row g, which needs n_rows >= G), and its slot
 * uniforms are stratified over the worlds of its root game (csrc/hsad_belief_world.h): W = n_worlds, w = world[g] (device int32
 * [G]), h(c) = hash(seed, group[g], c, 67), the policy's hash on stream 67 (group device int64 [G]: the root game's key).  Slot i:
 *   a_i = the first cand_k = 1 + ((h(16 + 8 i + k) (W - 1)) >> 32), k = 0 .. 7, with gcd(cand_k, W) == 1; 1 if there is none
 *   o_i = (h(2 i) W) >> 32;   s_i = (a_i w + o_i) mod W;   j_i = h((1 << 8) | i) >> 8  (the same in every world)
 *   k_i = ((s_i << 24) + j_i) / W  (uint64);   u_i = k_i << 8
 * and the hand is hsad_belief_tail's sample mode under u_0 .. u_4.  w -> s_i is a bijection of [0, W) for every slot: the W worlds
 * of a group fall into each of the W equal parts of every slot's conditional distribution exactly once, and -- the jitter j_i being
 * one per group and slot -- a slot's W points are a lattice of spacing 1 / W: any interval of length p holds floor(W p) or
 * ceil(W p) of them (slot 0's conditional is the same in all worlds of a group, so the number of them that hold type t there is
 * within 1 of W p_0[t]); one world alone is a plain draw from the belief (its stratum and the jitter are uniform), and W = 1 is
 * one.  The result depends on (seed, group[g], world[g]), the logits row and the game's state only: not on the slot g.  Skip rules, observe pass and the sad = 1 precondition are hsad_env_determinize_belief's.  A game is LEFT ALONE
 * -- state and rows, status 0, logp = logp0 = 0 -- when it is skipped, when row[g] is outside [0, n_rows), when world[g] is outside
 * [0, W), or when its row has a non-finite logit on an occupied slot.  logp_out / logp0_out device float [G] or NULL: the sampled
 * hand's log-probability under the belief, and under the exact belief (all-zero logits); their difference is the log importance
 * ratio.  status_out device int32 [G] or NULL.  HSAD_ERR_INVALID: a null viewer / logits / group / world, ldz < 25 H, n_rows < 1,
 * n_worlds outside [1, 2^20], hands of more than 5 slots; HSAD_ERR_STATE: the env's outputs are not bound.  No float atomics.
 * Launch-only. */
int hsad_env_determinize_belief_worlds(hsad_env* env, const int32_t* viewer, const float* logits, int ldz, int n_rows, const int32_t* row,
                                       const int64_t* group, const int32_t* world, int n_worlds, uint64_t seed, float* logp_out,
                                       float* logp0_out, int32_t* status_out, void* stream);

/* hsad_env_playout_random: up to max_iter iterations of random-legal policy -> step for every game that is started and not
 * finished, in one launch.  A finished game is left alone (no restart, no error, no counter advance); a live game's trajectory --
 * actions in a / greedy_a, state, draws -- is that of hsad_env_policy_random + hsad_env_step.  NO observation rows are written
 * (nothing consumes them; the launch is bound by game logic, not by HBM): priv_s / legal_move / own_hand / eps / reward and the
 * packed rows are STALE until the next hsad_env_fork, hsad_env_reset or hsad_env_step rewrites them.  `terminal`, hsad_env_query and
 * the masks hsad_env_policy_random reads are current.  Every workgroup bounds its own work (max_iter) and waits for no other.
 * _keyed: key (device int64 [G], NULL = the game index) replaces the game index in the policy's hash, so that a game's playout
 * does not depend on the slot it sits in. */
int hsad_env_playout_random(hsad_env* env, int max_iter, uint64_t policy_seed, int64_t* a, int64_t* greedy_a, void* stream);
int hsad_env_playout_random_keyed(hsad_env* env, int max_iter, uint64_t policy_seed, const int64_t* key, int64_t* a, int64_t* greedy_a,
                                  void* stream);

/* ---- Rule-list bots: a hand-coded Hanabi policy evaluated on the state planes on the device.  A bot is an ordered list of at most
 * HSAD_RULE_MAX_RULES rules; the first rule that fires gives the action, and if none fires the action is the lowest set bit of the
 * seat's legal mask.  Pure integer logic: every result is exact.  This text is the specification (csrc/hsad_rulebot.h follows it,
 * tests/rulebot_ref.py restates it); the rule names echo rule-based agents of the Hanabi literature, but no fidelity to any published
 * bot is claimed.
 *
 * The bot of seat p reads only what p may see: full[t] (copies of card type t = colour * 5 + rank under the env's rules, 0 outside
 * them), fireworks fw[c], discards, info, life, deck size, the other seats' cards with their knowledge words, and for its own slots
 * only the plausible-colour / plausible-rank masks and the hinted flags -- never its own cards.  Definitions:
 *   pool[t]   = deck count + copies in p's own hand (the pool of hsad_env_determinize);
 *   compat_i  = colour(t) and rank(t) both plausible for own slot i;   n_i = sum_t pool[t] compat_i[t]  (>= 1 in a valid position);
 *   playable(t): rank == fw[c];   dead(t): rank < fw[c], or some rank r' with fw[c] <= r' < rank has discards[c*5+r'] == full[c*5+r'];
 *   play_i, dead_i = the sum of n_i restricted to playable / dead types;
 *   a card in another hand is PUBLICLY KNOWN X when every type with full[t] > 0 in that slot's compat mask is X;
 *   scans over the partners' cards go by target offset 1 .. P-1, then by slot ascending, and the first hit wins;
 *   THE HINT FOR a card: the rank hint if that slot's plausible-rank mask has more than one bit, otherwise the colour hint if its
 *   plausible-colour mask has more than one bit; if both masks are singletons the card does not qualify and the scan goes on;
 *   every hint rule needs info > 0, every discard rule needs info < max_information_tokens;
 *   ratios are compared by integer cross-multiplication: x_i / n_i reaches k % iff x_i * 100 >= k * n_i, the best slot has the largest
 *   x_i / n_i (slot j beats slot b iff x_j * n_b > x_b * n_j), ties go to the lowest slot.
 * Rules (code, fires when -> action):
 *    1 PLAY_CERTAIN             lowest own slot with play_i == n_i -> play it
 *    2 PLAY_PROBABLE(k)         life > 1 and the best slot by play_i / n_i reaches k % -> play it
 *    3 PLAY_PROBABLE_ENDGAME(k) as 2, and the deck is empty
 *    4 HINT_PLAYABLE            first partner card that is playable and not publicly known playable (and qualifies) -> the hint for it
 *    5 HINT_USEFUL              first partner card that is not dead and qualifies -> the hint for it
 *    6 HINT_DEAD                first partner card that is dead and not publicly known dead (and qualifies) -> the hint for it
 *    7 HINT_RANDOM              hash pick among the hint bits of the legal mask (there is one)
 *    8 DISCARD_CERTAIN_DEAD     lowest own slot with dead_i == n_i -> discard it
 *    9 DISCARD_PROBABLE_DEAD(k) the best slot by dead_i / n_i reaches k % -> discard it
 *   10 DISCARD_UNHINTED_OLDEST  lowest own slot with neither hinted flag set -> discard it
 *   11 DISCARD_OLDEST           -> discard slot 0 (new cards are appended: slot 0 is the oldest)
 *   12 DISCARD_RANDOM           hash pick among the discard bits of the legal mask
 *   13 LEGAL_RANDOM             hash pick over the whole legal mask
 * k is 0 .. 100 for codes 2, 3 and 9 and must be 0 for every other code.  Action uids are those of the legal_move row: discard slot i
 * = i, play slot i = H + i, colour hint = 2H + (o-1) C + colour, rank hint = 2H + (P-1) C + (o-1) R + rank (o the target offset), noop
 * = A - 1; with shuffle_color a colour hint names the colour through the ACTOR's permutation, as its legal_move row does.  A seat that
 * is not on turn gets the noop.  greedy_a = a.  A hash pick is hsad_env_policy_random's: the k-th set bit, k = h % popcount, with
 *   h = hash(seed, key, counter, 128 + 16 p + j),   j = the rule's index in the list
 * (the random policy owns streams 0 .. 2P-1, the samplers 64 and 65); counter is the game's policy counter, read once and
 * incremented once per policy call, as hsad_env_policy_random does; key is key[g], or g when key == NULL.
 *
 * hsad_env_policy_rule: one policy call on the env's current state.  rules: HOST array [n_bot][HSAD_RULE_MAX_RULES] (bot b's list is
 * rules[b * 8 .. b * 8 + n_rules[b])); n_rules HOST int32 [n_bot].  seat_bot DEVICE int32 [G * P]: the bot that plays row g * P + p;
 * -1 leaves that row of a / greedy_a untouched.  A game whose P entries are all -1 is not touched at all (its counter included);
 * every other game's counter advances by one.  An entry below -1 or >= n_bot leaves the row alone and is counted in the env's error
 * log (code 7).  greedy_a may be NULL.  Reads the state planes only (no bound output is needed beyond hsad_env_bind_outputs).
 *
 * hsad_env_playout_rule: hsad_env_playout_random with the bots in place of the random pick: up to max_iter iterations of policy ->
 * step for every live game in one launch, finished games left alone (no counter advance), no observation rows written, `terminal`,
 * hsad_env_query and the legal masks current afterwards.  seat_bot_of_seat HOST int32 [P]: the bot of each seat, the same in every
 * game.  A live game's trajectory is that of hsad_env_policy_rule + hsad_env_step.  Refused while the env holds a deal script.
 *
 * Both return HSAD_ERR_INVALID with a message, before anything is launched, for: n_bot outside 1 .. HSAD_RULE_MAX_BOTS, an n_rules
 * entry outside 1 .. HSAD_RULE_MAX_RULES, an unknown rule code, k out of range, a seat_bot_of_seat entry outside 0 .. n_bot-1, more
 * than 5 players.  Launch-only. */
enum {
  HSAD_RULE_PLAY_CERTAIN = 1,
  HSAD_RULE_PLAY_PROBABLE = 2,
  HSAD_RULE_PLAY_PROBABLE_ENDGAME = 3,
  HSAD_RULE_HINT_PLAYABLE = 4,
  HSAD_RULE_HINT_USEFUL = 5,
  HSAD_RULE_HINT_DEAD = 6,
  HSAD_RULE_HINT_RANDOM = 7,
  HSAD_RULE_DISCARD_CERTAIN_DEAD = 8,
  HSAD_RULE_DISCARD_PROBABLE_DEAD = 9,
  HSAD_RULE_DISCARD_UNHINTED_OLDEST = 10,
  HSAD_RULE_DISCARD_OLDEST = 11,
  HSAD_RULE_DISCARD_RANDOM = 12,
  HSAD_RULE_LEGAL_RANDOM = 13,
  HSAD_RULE_MAX_RULES = 8,
  HSAD_RULE_MAX_BOTS = 8
};
typedef struct hsad_rule {
  int32_t code;
  int32_t k;
} hsad_rule;
int hsad_env_policy_rule(hsad_env* env, const hsad_rule* rules, const int32_t* n_rules, int n_bot, const int32_t* seat_bot, uint64_t seed,
                         const int64_t* key, int64_t* a, int64_t* greedy_a, void* stream);
int hsad_env_playout_rule(hsad_env* env, int max_iter, const hsad_rule* rules, const int32_t* n_rules, int n_bot,
                          const int32_t* seat_bot_of_seat, uint64_t seed, const int64_t* key, int64_t* a, int64_t* greedy_a, void* stream);

/* hsad_env_rewind_scripted: start games again from a deal somebody else chose.  script device uint8 [G, 52]: card types
 * (colour * 5 + rank) in deal order, the layout of the deck history (hsad_env_deck_history rows padded to 52); count device int32
 * [G]: how many deals of game g are scripted.  Every game with count[g] > 0 that is started goes back to what a fresh deal leaves --
 * full deck counts less the hands, empty discards and fireworks, full tokens, step 0, not terminated, cleared knowledge and last
 * move -- with the hands dealt from script[g, 0 .. P * H) in deal order (seat 0's H cards first).  What hsad_env_reset drew from the
 * generator is kept: the eps choice, the colour permutations, the generator's words, draw counter and look-ahead; so are the policy
 * counter and the last score.  Games with count[g] <= 0, and games that were never started, are left alone.  The rows of the rewound
 * games are rewritten by the observe pass (SAD section all-zero, reward 0, terminal 0).  The script must be a legal deal order:
 * P * H <= count[g] <= deck size, and every card a type the full deck still holds after the cards before it; otherwise the game is
 * left alone and counted in the error log (code 5).  The env copies the script (the caller's buffers may be reused at once).
 * From then on, while a game's deal index (deck size - cards left) is below count[g], hsad_env_step deals script[g, index] and
 * consumes NO generator draw; past the script it deals from the generator as ever.  hsad_env_fork copies the deal index with the
 * state; the script stays with the env it was given to (a game forked INTO a scripted env continues on that env's script; a scripted
 * card its deck does not hold is logged as code 5 and dealt from the generator).  hsad_env_reset and hsad_env_reseed clear the
 * script of every game.  An env that never received a script runs the very step, reset and rollout kernels it ran before this call
 * existed: the scripted deal is a separate instantiation of the step kernel, selected only after this call.  While an env holds a
 * script, hsad_env_rollout_random and hsad_env_playout_random are refused (HSAD_ERR_STATE).  Launch-only. */
int hsad_env_rewind_scripted(hsad_env* env, const uint8_t* script, const int32_t* count, void* stream);

/* The SAD greedy-action section of an observation as a value that can be logged and shown again.  It is no function of the state
 * (hsad_env_fork) -- and in a replayed world it is no function of that world either: what every seat SAW of a greedy action was
 * computed from the true cards (the card of a greedy play, the slots a greedy hint touches), whatever hand a sampled world holds.
 * hsad_env_sad_section: out device int64 [G * P] = the section of the env's currently bound rows (float32 or bit words), bit i =
 * column F - section length + i; all zero with sad = 0.
 * hsad_env_observe_sad: the observe pass of hsad_env_fork for every game g with 0 <= src_index[g] < G_src (device int32 [G]): all
 * bound rows of game g are rewritten from its state (reward = 0, terminal = the state's bit) with the section of seat p taken from
 * sad[src_index[g] * P + p] (device int64 [G_src * P]).  Other games keep their rows.  A no-op with sad = 0.  Launch-only. */
int hsad_env_sad_section(hsad_env* env, int64_t* out, void* stream);
int hsad_env_observe_sad(hsad_env* env, const int32_t* src_index, int G_src, const int64_t* sad, void* stream);

/* ---- Positions in and out of an env: set one up, save the games, take them back.  Both directions below are launch-only, act per
 * game, and check on the device before they write: a game whose input is refused is left alone -- state, generator, rows -- gets
 * the reason in its status word and is counted in the error log (code 6).  Nothing below changes what any earlier call computes.
 *
 * Why a position is refused, as bits of the status word.  The first eight are position_valid (csrc/hsad_position.h), the check both
 * calls share: it admits exactly the positions from which the step, the row builder, the legal-move masks, the deal, the belief
 * kernels and the playout index in range and keep every card accounted for. */
enum {
  HSAD_POS_CONSERVATION = 1,  /* for some card type: deck + discards + copies in hands + (its colour's firework > its rank) differs
                                 from the full deck's count; the deck-size field is not the sum of the deck counts; a card, a count
                                 or a firework sits in a colour >= colors or a rank >= ranks */
  HSAD_POS_BOARD = 2,         /* a firework > ranks; info > max_information_tokens; life > max_life_tokens; cur_player outside
                                 [0, P); next_non_chance_player != (cur_player + 1) % P; turns_to_play > P, or != P while the deck
                                 holds a card */
  HSAD_POS_HANDS = 4,         /* occupied slots not contiguous from 0; a length other than H, or H - 1 on an empty deck; more
                                 short hands than P - turns_to_play (each move on an empty deck takes one turn) */
  HSAD_POS_KNOWLEDGE = 8,     /* a plausible-colour / -rank mask that is empty, leaves the rules' colours / ranks or excludes the
                                 card's own; a hinted colour / rank (>= 0) that is not the card's or whose mask is not that one bit */
  HSAD_POS_LASTMOVE = 16,     /* last move: type outside 0..4, player >= P, target offset outside 1..P-1 (hints), colour >= colors,
                                 rank >= ranks, card index >= H, reveal mask >= 2^H.  Only what the encoder indexes with: whether
                                 the move fits the rest of the position is not checked and cannot be */
  HSAD_POS_STEP = 32,         /* num_step > 255, or > max_len when max_len > 0 */
  HSAD_POS_PERM = 64,         /* a colour permutation that is none of 0..4, moves a colour >= colors, whose inverse is not its
                                 inverse, or that is not the identity with shuffle_color off */
  HSAD_POS_TERMINAL = 128,    /* the position is finished: life < 1, every firework complete, turns_to_play < 1, or num_step ==
                                 max_len > 0.  A finished position is held to what a final move leaves, which no deal follows: the
                                 mover's hand may be short over a non-empty deck, and then cur_player is -1 and
                                 next_non_chance_player the seat after the mover */
  HSAD_POS_FIELD = 256,       /* import: a record word does not fit the bit field that holds it (reported alone: the record is not
                                 looked at further) */
  HSAD_POS_NO_GENERATOR = 512,/* import with seeds == NULL into a game that was never started: it has no generator to keep */
  HSAD_POS_LOOKAHEAD = 1024,  /* restore: look-ahead count > 2 */
  HSAD_POS_HISTORY = 2048,    /* restore: a deck-history or script card >= 25; a script count outside {0} and [P * H, deck size] */
  HSAD_POS_SCRIPT = 4096,     /* restore: the script's remaining deals name a card the record's deck does not hold */
  HSAD_POS_RECORD = 8192      /* restore: the record's terminated bit disagrees with its position */
};

/* hsad_env_import_state: game g with take[g] != 0 (device uint8 [G]) becomes the position states[g] (device int32
 * [G, hsad_env_state_words()], the layout hsad_env_export_state writes), live: started, not terminated, last score from word 74.
 * status (device int32 [G] or NULL): -1 for take[g] == 0 (game untouched), 0 imported, else the HSAD_POS_* flags (game untouched,
 * error log code 6).  A finished position is refused with HSAD_POS_TERMINAL.  Record fields the last move's type does not use,
 * the knowledge words of empty slots (card -1) and word 73 are ignored.
 * Generator: seeds (device int32 [G]) gives game g std::mt19937(seeds[g]) with no draw consumed and an empty look-ahead, exactly
 * hsad_env_fork's seeding; seeds == NULL keeps the game's generator, draw counter and look-ahead (HSAD_POS_NO_GENERATOR for a game
 * that was never started).  eps (device float [G, P]) sets the eps plane; NULL keeps it (0 for a never-started game).  The policy
 * counter is kept.  The cards of an imported position have no deal order: the game's deck-history row is cleared (the cards
 * hsad_env_deck_history returns for it are 0 until the next reset deals afresh) and, while the env holds a deal script, the game's
 * script is dropped -- the scripted-env rules apply unchanged to the other games.  The rows of the imported games are rewritten by
 * the observe pass as after hsad_env_rewind_scripted: SAD section all-zero, reward 0, terminal 0.  Launch-only. */
int hsad_env_import_state(hsad_env* env, const int32_t* states, const uint8_t* take, const int32_t* seeds, const float* eps,
                          int32_t* status, void* stream);

/* A snapshot is G fixed-size records in device memory, one per game, holding everything that decides what the game does and shows
 * next.  Record of 32-bit words, with npl = 10 + 6 P:
 *   [0, npl)            the state planes (board, hands, knowledge, eps, colour permutations, draw counter, look-ahead)
 *   [npl]               the policy counter
 *   [npl + 1, npl + 625) the 624 generator words
 *   then 13 words       the deck-history row (52 bytes)              -- only if the env tracks the deck history
 *   then 13 + 1 words   the deal-script row (52 bytes) and its count -- only if the env holds a deal script
 *   then 2 P words      the SAD section of each seat's current row (low word first; hsad_env_sad_section's value)
 * Size and offsets depend on (P, track_deck_history, script held) only; hsad_env_snapshot_record_bytes gives the size as the env
 * stands.  Pacing, timing and trace state is not game state and is not recorded; no rollout launch carries a per-game word into
 * the next that is not derived from the planes and the rows.  The records are opaque and exact: bytes may be copied, stored and
 * loaded by another process.  hsad_env_snapshot needs the env's observation rows (float32 or bit words) with sad = 1.
 * hsad_env_restore: dst game j becomes record src_index[j] (device int32 [G]) of `in` (G_src records of record_bytes each);
 * src_index == NULL is the identity and needs G_src == G; -1 leaves game j alone (status -1); another value outside [0, G_src)
 * too, counted as code 4.  record_bytes must be this env's record size with or without a deal script (HSAD_ERR_INVALID otherwise,
 * before anything is launched): records with a script make the env hold one (as hsad_env_rewind_scripted does), records without
 * clear the restored games' scripts.  Each record is read once and checked before a word of its game is written: a started record
 * must pass position_valid (a finished game is part of an env: HSAD_POS_TERMINAL is allowed, and must agree with the record's
 * terminated bit) and the HSAD_POS_LOOKAHEAD / _HISTORY / _SCRIPT checks; a never-started record is restored as it is.  Every
 * generator index is derived from the draw counter modulo 624, so any counter is in range.  A refused record leaves its game
 * alone: status = its flags, code 6.  The rows of the restored games are rewritten by the observe pass with the recorded SAD
 * section: every bound row, legal moves, own hand and eps are what the env showed when the snapshot was taken, bit for bit (given
 * that its rows were current then: hsad_env_playout_random leaves them stale); reward = 0, terminal = the state's bit. */
int64_t hsad_env_snapshot_record_bytes(const hsad_env* env);
int hsad_env_snapshot(hsad_env* env, void* out, void* stream);
int hsad_env_restore(hsad_env* env, const void* in, int64_t record_bytes, int G_src, const int32_t* src_index, int32_t* status,
                     void* stream);


/* ------------------------------------------------------------------------------------------
 * Device-resident sequence replay and actor buffers.
 * Replaces rela::PrioritizedReplay<RNNTransition> / ConcurrentQueue (rela/prioritized_replay.h:15-361),
 * RNNTransition::makeBatch (rela/transition.cc:160-202), MultiStepBuffer and R2D2Buffer
 * (rela/transition_buffer.h:8-227) and aggregatePriority (rela/r2d2_actor.h:10-21).
 *
 * A transition is described by n_fields per-step "fields" (the entries of the reference's obs and
 * action TensorDicts, e.g. priv_s, legal_move, eps, own_hand, a, greedy_a); reward, terminal,
 * bootstrap and seq_len are implicit.  All tensor arguments are device pointers.
 * ------------------------------------------------------------------------------------------ */
/* HSAD_BITS: values that are exactly 0.0f / 1.0f at the API (float32 tensors), stored as ONE BIT each -- every plane of the
 * Hanabi observation, the legal-move mask and the own-hand target are (cpp/hanabi_env.cc:115-205).  dtype = HSAD_BITS |
 * (segments << 8): `segments` equal parts (the players of a VDN row), each starting on a 64-bit word.  Storing a value that
 * is neither 0 nor 1 is counted by hsad_replay_error_count (the sequence writer's count joins it at the next flush). */
typedef enum { HSAD_F32 = 0, HSAD_I64 = 1, HSAD_U8 = 2, HSAD_BITS = 3 } hsad_dtype;
/* what hsad_replay_sample writes for a bit field: float32 [width] | bf16 [segments][ld] zero-padded (the learner's GEMM operand,
 * no cast pass) | the stored 64-bit words */
typedef enum { HSAD_BITS_AS_F32 = 0, HSAD_BITS_AS_BF16 = 1, HSAD_BITS_AS_RAW = 2 } hsad_bits_out;
typedef struct hsad_field {
  int32_t width; /* elements per step (per env)          */
  int32_t dtype; /* hsad_dtype                            */
} hsad_field;

/* rela::aggregatePriority: priority float32 [T,B], seq_len float32 [B] -> out float32 [B]
 * = eta * max_t(p*mask) + (1-eta) * sum_t(p*mask) / seq_len. */
int hsad_aggregate_priority(const float* priority, const float* seq_len, int T, int B, float eta, float* out,
                            void* stream);

typedef struct hsad_replay hsad_replay;

/* RNNPrioritizedReplay(capacity, seed, alpha, beta, prefetch) (rela/pybind.cc:46-58).  Storage is a ring
 * of int(1.25*capacity) sequences of seq_len steps in HBM; prefetch is accepted for signature
 * compatibility and ignored (sampling is a stream-ordered kernel, there is nothing to prefetch). */
int hsad_replay_create(int capacity, int seed, float alpha, float beta, int prefetch, int seq_len, int n_fields,
                       const hsad_field* fields, int device, hsad_replay** out);
void hsad_replay_destroy(hsad_replay* r);
int64_t hsad_replay_bytes(const hsad_replay* r);

/* PrioritizedReplay::add(vector<RNNTransition>, priority): n sequences, fields[k] -> [n, T, width_k],
 * reward/bootstrap float32 [n,T], terminal uint8 [n,T], seq_len/priority float32 [n].  Weight = priority^alpha.
 * n_dev (may be NULL): device int32 holding the actual count (<= n) for sync-free producers.
 * Where the reference would block the producer on a full ring (blockAppend) until sample() pops, add() evicts the
 * oldest entries itself to make room (same bookkeeping as blockPop); only n > ring is an error. */
int hsad_replay_add(hsad_replay* r, int n, const void* const* fields, const float* reward, const uint8_t* terminal,
                    const float* bootstrap, const float* seq_len, const float* priority, const int32_t* n_dev,
                    void* stream);

/* PrioritizedReplay::sample (+ makeBatch): stratified draw of `batch` sequences (duplicates possible),
 * out_fields[k] -> [T, batch, width_k], reward/bootstrap float32 [T,batch], terminal uint8 [T,batch],
 * seq_len float32 [batch], weight float32 [batch] = (N*w/sum)^-beta / max; evicts the oldest entries when
 * size > capacity.  Must alternate with hsad_replay_update_priority like the reference (prioritized_replay.h:209-212). */
int hsad_replay_sample(hsad_replay* r, int batch, void* const* out_fields, float* reward, uint8_t* terminal,
                       float* bootstrap, float* seq_len, float* weight, void* stream);
int hsad_replay_update_priority(hsad_replay* r, const float* priority, int batch, void* stream);
/* Sharded replay (one shard per GPU).  The reference's stratified draw (prioritized_replay.h:291-334) is
 * taken over the CONCATENATION of the shards: rank-0's generator supplies the canonical uniforms
 * (hsad_replay_draw_canonical = the generate_canonical<float,24> stream sample() would consume), every shard reports its
 * running weight sum / size (hsad_replay_priority_sum; synchronises), and serves the positions that fall inside its own
 * slice with hsad_replay_sample_at: targets_host[i] = global position - weight of the shards before this one (host float32,
 * n may be 0: only the eviction bookkeeping of sample() runs).  raw_weight [n] receives w_i = priority^alpha of the drawn
 * elements; the caller forms (N*w/sum)^-beta / max over the assembled batch.  Alternates with
 * hsad_replay_update_priority(n) like hsad_replay_sample.  Host-side choreography: hanabi_sad_amd/dist.py. */
int hsad_replay_priority_sum(hsad_replay* r, double* sum, int32_t* size);
int hsad_replay_draw_canonical(hsad_replay* r, int n, float* out_host);
int hsad_replay_sample_at(hsad_replay* r, int n, const float* targets_host, void* const* out_fields, float* reward,
                          uint8_t* terminal, float* bootstrap, float* seq_len, float* raw_weight, void* stream);
/* size() / numAdd(): synchronise the stream the producers used, then read the device counters. */
int hsad_replay_size(hsad_replay* r, int32_t* size, int32_t* num_add);
/* get(idx): element idx counted from the ring head; out_fields[k] -> [T, width_k] */
int hsad_replay_get(hsad_replay* r, int idx, void* const* out_fields, float* reward, uint8_t* terminal,
                    float* bootstrap, float* seq_len, void* stream);
/* physical ring slots of the last sample (device int32 [batch]); debugging / tests */
int hsad_replay_last_ids(hsad_replay* r, int32_t* out, int batch, void* stream);

/* The same sharded draw WITHOUT host round trips (every argument a device pointer; the exchange between the calls is the host's:
 * RCCL through torch.distributed in hanabi_sad_amd/dist.py ReplayLink), so an actor rank serves a learner's request between two of
 * its own steps and the learner never stalls the actors:
 *   hsad_replay_stats         (sum, size) of this shard as two doubles -> all-gathered into all_stats [world][2]
 *   hsad_replay_serve         canon [B] = the learner's canonical uniforms.  Computes the reference's stratified positions over the
 *                             concatenation of the shards (prioritized_replay.h:300-305), owner_out[i] = shard of position i, draws
 *                             the positions this shard owns and writes those sequences, in batch order, into slots 0.. of wire_out
 *                             ([B][hsad_replay_wire_bytes]: stored rows incl. the bit-packed observation + reward / bootstrap /
 *                             terminal / seq_len / raw weight).  The draw joins the outstanding queue (hsad_replay_set_outstanding).
 *   hsad_replay_update_owned  priority [B] of a whole batch + that draw's owner[]: answers the OLDEST outstanding draw with the
 *                             priorities of the positions this shard owned
 *   hsad_replay_assemble      learner: wire_all [world][B][wire_bytes] (every rank's buffer) + owner[] -> the batch tensors exactly as
 *                             hsad_replay_sample lays them out (bit fields per hsad_replay_set_field_output) + raw weights [B] */
int hsad_replay_stats(hsad_replay* r, double* out2, void* stream);
int hsad_replay_wire_bytes(const hsad_replay* r);
int hsad_replay_serve(hsad_replay* r, int batch, const float* canon, const double* all_stats, int world, int rank, int32_t* owner_out,
                      uint8_t* wire_out, void* stream);
int hsad_replay_update_owned(hsad_replay* r, int batch, const float* priority, const int32_t* owner, int rank, void* stream);
int hsad_replay_assemble(hsad_replay* r, int batch, int world, const uint8_t* wire_all, const int32_t* owner, void* const* out_fields,
                         float* reward, uint8_t* terminal, float* bootstrap, float* seq_len, float* raw_weight, void* stream);
/* Drawn batches that may wait for their priorities at once (1..8, default 1 = strict alternation).  The reference's
 * prefetch queue (prioritized_replay.h:232-262, prefetch = 3 in selfplay.py) draws up to `prefetch` batches before the
 * priorities of the batches in training are written back; with depth k, hsad_replay_update_priority answers the OLDEST
 * outstanding draw, and elements evicted since their draw are skipped as in ConcurrentQueue::update.  A draw into a full
 * queue replaces the newest entry.  HSAD_ERR_STATE while draws are outstanding. */
int hsad_replay_set_outstanding(hsad_replay* r, int depth);
/* Output format of bit field `field` in hsad_replay_sample / _sample_at (hsad_bits_out; ld = bf16 elements per segment row). */
int hsad_replay_set_field_output(hsad_replay* r, int field, int kind, int ld);
int hsad_replay_row_bytes(const hsad_replay* r);              /* bytes of one stored step                     */
int hsad_replay_field_bytes(const hsad_replay* r, int field); /* bytes of field `field` inside a stored step  */
int hsad_replay_error_count(hsad_replay* r, int32_t* count);
/* which contracts the violations counted by the last hsad_replay_error_count call broke (OR of 1 = add larger than the ring,
 * 2 = draw beyond the weight sum, 4 = update_priority without a matching draw, 8 = sequence writer / non-binary bit field) */
int hsad_replay_error_kinds(const hsad_replay* r);

typedef struct hsad_seqwriter hsad_seqwriter;

/* MultiStepBuffer(multi_step, num_envs, gamma) + R2D2Buffer(num_envs, ., multi_step, seq_len) for one actor. */
int hsad_seqwriter_create(int num_envs, int multi_step, float gamma, int seq_len, int n_fields,
                          const hsad_field* fields, int device, hsad_seqwriter** out);
void hsad_seqwriter_destroy(hsad_seqwriter* w);
/* MultiStepBuffer::pushObsAndAction: fields[k] -> [E, width_k] of the current step */
int hsad_seqwriter_push_obs_action(hsad_seqwriter* w, const void* const* fields, void* stream);
/* Bit fields in `field_mask` arrive in hsad_seqwriter_push_obs_action already as bit words (the stored format: per segment
 * ceil(width / segments / 64) uint64, LSB first) -- what hsad_env_bind_packed makes the env kernel write. */
int hsad_seqwriter_set_prepacked(hsad_seqwriter* w, uint32_t field_mask);
/* MultiStepBuffer::pushRewardAndTerminal: reward float32 [E], terminal uint8 [E] */
int hsad_seqwriter_push_reward_terminal(hsad_seqwriter* w, const float* reward, const uint8_t* terminal, void* stream);
/* the same from per-GAME values: row e gets reward[e / repeat], terminal[e / repeat] (IQL: repeat = players) */
int hsad_seqwriter_push_reward_terminal_rep(hsad_seqwriter* w, const float* reward, const uint8_t* terminal, int repeat, void* stream);
/* MultiStepBuffer::canPop (host-side count, no synchronisation) */
int hsad_seqwriter_can_pop(const hsad_seqwriter* w);
/* MultiStepBuffer::popTransition: n-step return / bootstrap / terminal of the oldest step -> float32/uint8 [E];
 * out_fields / out_next_fields (either may be NULL): obs+action of that step and obs of step +n, [E, width_k]. */
int hsad_seqwriter_pop_transition(hsad_seqwriter* w, void* const* out_fields, void* const* out_next_fields,
                                  float* reward, uint8_t* terminal, float* bootstrap, void* stream);
/* R2D2Buffer::push of the transition just popped, with its per-env priority float32 [E]; pads finished sequences. */
int hsad_seqwriter_push_sequence(hsad_seqwriter* w, const float* priority, void* stream);
/* R2D2Buffer::popTransition + aggregatePriority + PrioritizedReplay::add for every finished env (ascending env
 * order), entirely on the device; n_finished_dev (may be NULL) receives the count. */
/* push_reward_terminal_rep + pop_transition + hsad_nstep_priority + push_sequence of one thread-loop iteration as ONE launch (what
 * cpp/thread_loop.h:66-84 does per step through R2D2Actor::postAct, rela/r2d2_actor.h:101-172): needs the step's obs / action pushed and then
 * n + 1 steps in the history (hsad_seqwriter_step_tail_ready; otherwise HSAD_ERR_STATE -- use the four entry points), rows <= 256 bytes.
 * qa / target_qa [E] = Q_online(s_{t-n}, a_{t-n}) / Q_target(s_t, greedy_t); priority_out [E]; reward_out / bootstrap_out optional [E]. */
int hsad_seqwriter_step_tail(hsad_seqwriter* w, const float* reward, const uint8_t* terminal, int repeat, const float* qa, const float* target_qa,
                             int multi_step, double gamma, float* priority_out, float* reward_out, float* bootstrap_out, void* stream);
int hsad_seqwriter_step_tail_ready(const hsad_seqwriter* w);
int hsad_seqwriter_flush_to_replay(hsad_seqwriter* w, hsad_replay* r, float eta, int32_t* n_finished_dev, void* stream);

/* ------------------------------------------------------------------------------------------
 * R2D2 recurrent Q-network kernels (bf16 MFMA operands, fp32 accumulation / state / loss).
 * Replace what the reference gets from PyTorch + cuDNN for R2D2Net / R2D2Agent
 * (pyhanabi/r2d2.py:13-157, 383-499).  All pointers are device pointers; bf16 buffers are raw uint16.
 * ------------------------------------------------------------------------------------------ */
/* C[M,N] = A[M,K] * B[N,K]^T (+bias[N]) (ReLU): A,B bf16 row-major (lda/ldb multiples of 8, K multiple of 64,
 * zero padded), outputs fp32 C32 (optionally accumulated into) and/or bf16 C16.  nn.Linear forward. */
int hsad_gemm_nt_bf16(const void* A, int lda, const void* B, int ldb, int M, int N, int K, const float* bias,
                      float* C32, int ldc, void* C16, int ldc16, int relu, int accumulate, void* stream);
/* two problems of the same shape (A0 B0^T, A1 B1^T; both with bias / fp32 output / bf16 output or both without) as ONE launch: the
 * online / target pair of every forward GEMM of the learner.  Tile rounds: 2 x 2.5 -> 5. */
int hsad_gemm_nt_bf16_pair(const void* A0, const void* A1, int lda, const void* B0, const void* B1, int ldb, int M, int N, int K,
                           const float* bias0, const float* bias1, float* C32_0, float* C32_1, int ldc, void* C16_0, void* C16_1,
                           int ldc16, int relu, void* stream);
/* developer switch (default 1; env HSAD_GEMM_PP): bf16-output GEMMs of whole 256 x 256 tiles, at least one per CU, run on the
 * phase-interleaved 256 x 256 kernel (the fused cell kernel's operand stream with a plain epilogue) -- identical bits, 0 = the
 * 128 x 128 kernel everywhere */
int hsad_gemm_set_pp(int on);
/* fp32 [M,K] (row stride ld_src) -> bf16 [M,Kp] zero padded */
int hsad_cast_pad_bf16(const float* src, int M, int K, int ld_src, void* dst, int Kp, void* stream);
/* bf16 [R,C] -> [C,R] */
int hsad_transpose_bf16(const void* src, int R, int C, int ld_src, void* dst, int ld_dst, void* stream);
/* One LSTM layer over T steps (nn.LSTM semantics, gate order i,f,g,o).  gates fp32 [T,Bn,4H] holds the input
 * projection x W_ih^T + b_ih + b_hh on entry and the activated gates on exit, both in the gate-blocked column
 * layout (block nb of 32 units: columns nb*128 + gate*32 + u); Whh_blocked bf16 [4H,H] has its rows in the same
 * order.  h0/c0 fp32 [Bn,H] (h0 NULL = zeros).  Outputs hseq16 bf16 [T,Bn,H], cseq fp32 [T,Bn,H], hT fp32 [Bn,H]
 * (optional).  h0_16_scratch: bf16 [Bn,H].  sync_scratch (may be NULL): uint32 [(T+2)*ceil(Bn/32)+4]; when given and
 * the shape allows (H in {256,512}, Bn <= 512) the whole sequence runs as ONE persistent launch that keeps the
 * W_hh slices in LDS and exchanges h_t tiles through L2 (csrc/hsad_r2d2.hip); otherwise one launch per step.
 * keep_gates = 0 (inference; per-step kernels only): the activated gates are not written back.
 * The word after the counters is a STICKY timeout flag (zero the scratch once when allocating it; launches only
 * clear the counters); hsad_lstm_sync_timed_out() reports a bounded spin that gave up. */
int hsad_lstm_layer_forward(int T, int Bn, int H, float* gates, const void* Whh_blocked, const float* h0,
                            const float* c0, void* hseq16, float* cseq, void* h0_16_scratch, float* hT,
                            void* sync_scratch, int keep_gates, void* stream);
/* One LSTM cell step for inference (actors; T = 1, tens of thousands of rows) at GEMM speed: gates = [x | h_prev]
 * [W_ih | W_hh]^T + bias with the cell update in the epilogue -- the gate pre-activations never reach HBM.  h_prev16 is
 * the bf16 cast [Bn,H] of the fp32 state (hsad_cast_pad_bf16) and may not alias h_out16.  Column order "gate16": rows of Wcat_gate16 bf16 [4H, Kx+H] and bias_gate16 [4H]
 * come in groups of 64 = [i(16) f(16) g(16) o(16)] of 16 hidden units (row 64*ub + 16*gate + u <- nn.LSTM row gate*H +
 * 16*ub + u); x16 bf16 [Bn,Kx] (ld = ldx); c_prev / c_out / h_out32 fp32 [Bn,H] (c_out may be c_prev; c_out, h_out32 and
 * h_out16 are each optional -- a caller that only wants the layer's output, e.g. the target net of an actor, skips the state); h_out16 bf16 [Bn,H] optional
 * (the next layer's x). */
int hsad_lstm_cell_fused(int Bn, int H, int Kx, const void* x16, int ldx, const void* h_prev16, const void* Wcat_gate16,
                         const float* bias_gate16, const float* c_prev, float* c_out, float* h_out32, void* h_out16,
                         void* stream);
/* Two cells of the same shape in ONE launch: problem a and problem b (e.g. the online and the target net's layer of an acting step; b
 * typically with c_out / h_out32 NULL).  Same bits as two hsad_lstm_cell_fused calls, which is also the fallback when the
 * phase-interleaved 256 x 256 kernel does not apply (rows < 4096 or rows % 256 != 0). */
int hsad_lstm_cell_fused_pair(int Bn, int H, int Kx, int ldx, const void* x16_a, const void* x16_b, const void* h_prev16_a, const void* h_prev16_b,
                              const void* Wcat_a, const void* Wcat_b, const float* bias_a, const float* bias_b, const float* c_prev_a,
                              const float* c_prev_b, float* c_out_a, float* c_out_b, float* h_out32_a, float* h_out32_b, void* h_out16_a,
                              void* h_out16_b, void* stream);
/* Developer switch (tests, A/B tools): which kernel hsad_lstm_cell_fused launches.  tile: 0 by size (256 x 256 tiles from 4,096 rows on),
 * 128 | 256 forced; pp: 1 (default) the phase-interleaved k loop (lstm_cell_pp_kernel; rows % 256 == 0), 0 the one-barrier k loop,
 * 11 / 12 / 14 / 19 timing ablations of the former (garbage results).  All real variants give identical bits. */
int hsad_lstm_cell_set_variant(int tile, int pp);
/* testing: force_cross_xcd != 0 makes every persistent recurrence use the cross-XCD hand-off protocol even when its
 * workgroups are co-located (the default, 0, picks per group at start-up); results must not depend on it */
int hsad_lstm_set_exchange_mode(int force_cross_xcd);
/* testing: make one workgroup of a persistent recurrence launch late on purpose.  While set, every launch of `kernel` (HSAD_STALL_*)
 * copies the hook into its arguments; the one workgroup (record, row_block, unit_block) sleeps `microseconds` (at most 200; a bounded
 * delay, far below any wait's give-up) in step `step`, behind that step's counter wait and in front of its hand-off stores, and adds 1
 * to a device word.  record: the launch's own index -- fused forward net * nlayer + layer, wide BPTT the stage (0 top layer,
 * 1 projection, 2 lower layer, 3 sink), 32 x 32 BPTT the internal record.  kernel < 0 clears the hook.  Results must not change. */
#define HSAD_STALL_FWD 0
#define HSAD_STALL_BPTT_WIDE 1
#define HSAD_STALL_BPTT_32 2
int hsad_lstm_debug_stall(int kernel, int record, int row_block, int unit_block, int step, int microseconds);
/* the device word of hsad_lstm_debug_stall: stalls served since the last reset (synchronises the device) */
int hsad_lstm_debug_stall_fired(uint64_t* count, int reset);
/* developer phase timers of the persistent recurrences (100 MHz ticks summed over the steps of one workgroup; slots
 * 0-5 forward: wait, h loads, MFMA, cell update, publish, state stores; 8-11 backward: wait, loads+MFMA, cell backward,
 * publish); out16 may be NULL; reset != 0 clears them */
int hsad_lstm_debug_timing(uint64_t* out16, int reset);
int hsad_lstm_debug_timing32(uint64_t* out32, int reset);   /* + slots 16-31: the fused BPTT kernel (top layer 16-21, lower layer 24-29) */
/* phase timers of the FUSED persistent kernels (off by default: a stamp costs ~0.1 us of the ~5 us step it measures) */
int hsad_lstm_debug_enable(int enable);
/* enable = 2: per-step trace instead of the summed timers -- thread 0 of every workgroup of row block 0 of the fused recurrences
 * stamps s_memrealtime (100 MHz, chip-wide) at its phase boundaries; hsad_lstm_debug_trace copies the last launches' stamps
 * [kernel: 0 forward, 1 BPTT][record 6][unit block 16][step 96][stamp 12] (n_words must be 2*6*16*96*12) and clears them */
int hsad_lstm_debug_trace(uint64_t* out, size_t n_words);
/* test hook: n_wg workgroups (threads, lds_bytes each) resident on `stream` until *flag_host_mapped (pinned host word) != 0 or max_us --
 * the footprint of a posted communication kernel whose peer has not answered, next to the learner's whole-chip persistent launches */
int hsad_debug_resident_kernel(int n_wg, int threads, int lds_bytes, const void* flag_host_mapped, int max_us, void* stream);
/* measurement hook for the fused cell kernel (hsad_lstm_cell_fused, i.e. every LSTM layer of an acting step): while enabled, each
 * launch is bracketed by HIP events on its own stream; _read returns the average duration and FLOP of the launches recorded since
 * the last read (synchronises) and clears the record.  bench.py's actor roofline. */
int hsad_lstm_cell_timing(int enable);
int hsad_lstm_cell_timing_read(double* avg_ms, double* avg_flop, int32_t* launches);
/* the same for the bf16 GEMM: events around every launch while enabled; _read averages the launches of one shape */
int hsad_gemm_timing(int enable);
int hsad_gemm_timing_read(int M, int N, int K, double* avg_ms, int32_t* launches, int32_t* problems_per_launch);
/* reads the timeout word of a sync_scratch buffer used with T steps / Bn rows (synchronises the device) */
int hsad_lstm_sync_timed_out(const void* sync_scratch, int T, int Bn, int32_t* timed_out);
/* Dueling head + masked argmax (r2d2.py:106-131): heads fp32 [M,ldh] = [advantage(A) | value(1) | ...],
 * legal fp32 [M,A], action int64 [M] (may be NULL) -> q [M,A], qa [M], greedy int64 [M] (may be NULL).
 * scratch: fp32 [2 + ceil(M/256)].  On return scratch[1 + i] = min of q over rows [256 i, 256 i + 256) (what hsad_loss_tail folds);
 * scratch[0] = the global minimum, written only when a greedy output is asked for (nobody reads it otherwise). */
int hsad_q_head(const float* heads, int ldh, const float* legal, const int64_t* action, int M, int A, float* q,
                float* qa, int64_t* greedy, float* scratch, void* stream);
/* n-step double-DQN TD error, Huber loss, priorities (r2d2.py:403-428,472-478); all [T,B] fp32 except
 * seq_len/loss/weight [B].  dqa (may be NULL) receives d mean_b(weight_b*loss_b) / d online_qa. */
int hsad_td_loss(const float* online_qa, const float* target_qa, const float* reward, const float* bootstrap,
                 const float* seq_len, int T, int B, int multi_step, double gamma, float* err, float* priority,
                 float* loss, float* dqa, const float* weight, void* stream);
/* hsad_gemm_nt_bf16 with split-K (fp32 atomic accumulation into a pre-zeroed / running C32; for weight
 * gradients whose contraction dimension is T*B) and an optional ReLU-backward mask (output zeroed where
 * relu_mask16 <= 0). */
int hsad_gemm_nt_bf16_ex(const void* A, int lda, const void* B, int ldb, int M, int N, int K, const float* bias,
                         float* C32, int ldc, void* C16, int ldc16, int relu, int accumulate, int split_k,
                         const void* relu_mask16, int ldmask, const int32_t* row_map, void* stream);
/* (row_map, may be NULL: result row r lands in output row row_map[r] -- un-blocks the gate-blocked weight gradients) */
/* split-K without atomics (weight gradients: contraction over T*B): every K split writes its partial [M,N] into its own slab
 * of `workspace` (fp32 [split_k, M, N]) through the fast epilogue, then one pass sums the slabs into
 * C32[row_map ? row_map[r] : r] (overwritten).  N and ldc multiples of 4. */
int hsad_gemm_nt_bf16_splitk(const void* A, int lda, const void* B, int ldb, int M, int N, int K, int split_k, float* workspace,
                             float* C32, int ldc, const int32_t* row_map, void* stream);
/* the same, ADDED to C32 instead of overwriting it (slabs, then one adding pass: deterministic) -- a contraction that arrives in pieces */
int hsad_gemm_nt_bf16_splitk_acc(const void* A, int lda, const void* B, int ldb, int M, int N, int K, int split_k, float* workspace,
                                 float* C32, int ldc, const int32_t* row_map, void* stream);
/* Several split-K GEMMs C_i (+)= A_i B_i^T (fp32 out) as ONE launch of the 256 x 256 core plus ONE slab-summing pass: the weight
 * gradients of a learner update (reference: loss.backward() of pyhanabi/selfplay.py:226 -- dW = dG^T [x | h] for both LSTM layers and the
 * input layer, K = T x B = 10,240) are a handful of problems that are each too small to fill the chip.  Every item's K is cut into
 * split_k ranges (an even number of 64-deep k tiles each), every (problem, range, tile) is a work item of the same launch, partial
 * results go to `workspace` (sum over items of ranges x M x N floats: hsad_gemm_group_workspace_floats) and are added up in range order
 * (deterministic).  M a multiple of 256, N of 4, K of 128, lda / ldb of 8; B is read up to its row N - 1 only.  When the core does not
 * take one of the items (an M that is no multiple of 256; hsad_gemm_set_pp(0)), every item runs on the 128 x 128 kernel, one launch each,
 * over the SAME k ranges (the planned range length is handed to it: csrc/hsad_gemm_plan.h) into the same slabs: identical bits on
 * either path (tests/test_gemm_group_gpu.py). */
typedef struct hsad_gemm_group_item {
  const void* A;            /* bf16 [M, K], row stride lda */
  const void* B;            /* bf16 [N, K], row stride ldb */
  float* C;                 /* fp32 [M, >= n_out], row stride ldc (any) */
  const int32_t* row_map;   /* optional [M]: result row r is written to row row_map[r] of C */
  int32_t lda, ldb, ldc;
  int32_t M, N, K;
  int32_t n_out;            /* columns of the result that are written to C (<= N; the operands may be zero-padded past it) */
  int32_t split_k;
  int32_t accumulate;       /* C += instead of C = */
} hsad_gemm_group_item;
int64_t hsad_gemm_group_workspace_floats(int n, const hsad_gemm_group_item* items);
int hsad_gemm_nt_bf16_group_splitk(int n, const hsad_gemm_group_item* items, float* workspace, int64_t workspace_floats, void* stream);
/* hsad_transpose_bf16 that also accumulates (atomically) the column sums of src into colsum[col_map ? col_map[c] : c]
 * (and colsum2): the bias gradients come for free while the weight-gradient operand is transposed */
int hsad_transpose_bf16_colsum(const void* src, int R, int C, int ld_src, void* dst, int ld_dst, float* colsum, float* colsum2,
                               const int32_t* col_map, void* stream);
/* fp32 master weight [R,C] -> bf16 kernel operands in one pass: dst16[r][:] = src[perm ? perm[r] : r][:] and/or its
 * transpose dstT16[c][r] (either may be NULL; padding of the destinations is left untouched).  Replaces
 * `weight[perm].to(bfloat16)` + transpose after every optimizer step. */
int hsad_prepare_weight(const float* src, int R, int C, int ld_src, const int32_t* perm, void* dst16, int ld_dst,
                        void* dstT16, int ld_dstT, void* stream);
/* out[i] = a[perm[i]] + b[perm[i]] (b / perm may be NULL): the gate bias b_ih + b_hh in gate-blocked order */
int hsad_bias_sum_perm(const float* a, const float* b, const int32_t* perm, float* out, int n, void* stream);
/* the same, batched: every operand of a net re-derived in ONE launch (hsad_r2d2_net_refresh uses it).  begin, then up to 20
 * hsad_prepare_weight jobs, then up to 12 hsad_bias_sum_perm jobs (no weight job after a bias job), then launch.  The job list is
 * thread-local host state. */
int hsad_refresh_begin(void);
int hsad_refresh_add_weight(const float* src, int R, int C, int ld_src, const int32_t* perm, void* dst16, int ld_dst, void* dstT16,
                            int ld_dstT);
int hsad_refresh_add_bias(const float* a, const float* b, const int32_t* perm, float* out, int n);
int hsad_refresh_launch(void* stream);
/* BPTT through one LSTM layer (learner batches).  gates/cseq: saved by hsad_lstm_layer_forward; c0 (may be NULL =
 * zeros); WhhT_blocked bf16 [H,4H] = transpose of the gate-blocked W_hh; dO fp32 [T,Bn,H] (may be NULL).
 * Output dG16 bf16 [T+1,Bn,4H] (slot T is scratch): gradient wrt the gate pre-activations, gate-blocked.
 * sync_scratch: as for hsad_lstm_layer_forward (NULL = one launch per step). */
int hsad_lstm_layer_backward(int T, int Bn, int H, const float* gates, const float* cseq, const float* c0,
                             const void* WhhT_blocked, const float* dO, void* dG16, float* dc_scratch,
                             void* sync_scratch, void* stream);
/* Gradient wrt the head outputs [advantage | value | aux logits] from d(loss)/d(qa) and the aux cross-entropy
 * (r2d2.py:124-153); pred_scale = pred_weight / B (0 disables the aux part).  out16 bf16 [M, ldo]. */
int hsad_heads_backward(const float* dqa, const float* legal, const int64_t* action, const float* heads, int ldh,
                        const float* own_hand, const float* weight, int M, int B, int A, int NP, float pred_scale,
                        void* out16, int ldo, void* stream);
/* aux own-hand cross-entropy summed over time (cross_entropy, r2d2.py:133-153): xent_sum fp32 [B] */
int hsad_aux_xent(const float* heads, int ldh, const float* own_hand, int T, int B, int A, int NP, float* xent_sum,
                  void* stream);
/* Everything between the online Q-head and BPTT of an IQL learner update in ONE launch (one block per sequence): global min(q) from the
 * block minima hsad_q_head left in its scratch (scratch + 1, (M + 255) / 256 of them) -> greedy action (r2d2.py:113-115) -> Q_target(s, greedy)
 * from the target net's heads -> n-step TD error, Huber loss, priority, d loss / d qa (hsad_td_loss) -> auxiliary cross-entropy
 * (hsad_aux_xent; loss += pred_weight * xent) -> d loss / d heads rows bf16 [M, ldo] (hsad_heads_backward; dheads16 NULL = no gradient).
 * Same arithmetic and summation order as those entry points: bit-identical results, six launches fewer per update. */
int hsad_loss_tail(const float* heads, const float* heads_t, int ldh, const float* legal, const float* q_online, const float* online_qa,
                   const float* block_min, int n_block_min, const float* reward, const float* bootstrap, const float* seq_len,
                   const float* weight, const float* own_hand, const int64_t* action, int T, int B, int A, int NP, int multi_step, double gamma,
                   float pred_weight, int64_t* greedy, float* target_qa, float* err, float* priority, float* loss, float* xent_sum, float* dqa,
                   void* dheads16, int ldo, void* stream);
/* Behaviour cloning on the head outputs, one launch (IQL layout, any T): row m = t B + b, z_j = heads[m ldh + j] (j < A), legal 0 / 1 [M, A],
 * action [M], valid = t < seq_len[b].  Policy = softmax over the LEGAL advantages (= softmax over legal Q under the dueling head; its argmax is
 * the greedy action of hsad_r2d2_act).  loss[b] = sum_t xent_t in ascending t, xent = log sum_legal exp(z_j - max) - (z_act - max);
 * decisions[b] = valid steps with >= 2 legal actions, hits[b] = those whose legal argmax (ties: lowest index) is the action; bad[b] = valid
 * steps whose action is out of range or illegal (they contribute nothing).  dheads16 (NULL = no gradient): bf16 [M, ldo],
 * (weight[b] / B) (softmax_j - delta_{j, act}) in the A advantage columns, 0 in the value column (cloning gives the value no gradient) and up to
 * ldo; all-zero rows for invalid, bad and single-legal steps (a single legal action is exactly xent = 0).  No float atomics. */
int hsad_clone_tail(const float* heads, int ldh, const float* legal, const int64_t* action, const float* seq_len, const float* weight, int T, int B,
                    int A, float* loss, int32_t* hits, int32_t* decisions, int32_t* bad, void* dheads16, int ldo, void* stream);
/* hsad_clone_tail with a value term, one launch: next to the cross-entropy (loss, hits, decisions, bad as there) every valid row that is not bad
 * regresses the dueling Q of the recorded action on ret [M], the return-to-go of the step: v = heads[m ldh + A], al_j = z_j l_j,
 * q = v + al_act - (sum_j al_j) / A, e = ret[m] - q, Huber term |e| < 1 ? e e / 2 : |e| - 1/2 (the TD loss's), g = -clamp(e, -1, 1).
 * vloss[b] = sum_t Huber_t in ascending t; steps[b] = valid rows that are not bad (single-legal rows included: the off-turn no-op has a Q too).
 * dheads16 (NULL = no gradient): bf16 [M, ldo], with s = weight[b] / B
 *   column j < A: s (policy_weight (softmax_j - delta_{j, act}) [>= 2 legal] + value_weight g l_j (delta_{j, act} - 1/A)), summed in fp32, rounded once
 *   column A: s value_weight g; columns A + 1 .. ldo - 1: 0; invalid and bad rows: all-zero bits (they read neither ret nor the logits).
 * value_weight == 0 reads no ret and writes no vloss (both may be NULL); with policy_weight == 1 loss, hits, decisions, bad and dheads16 then
 * have the bits of hsad_clone_tail.  Refused: what hsad_clone_tail refuses, value_weight != 0 without ret, vloss or a value column (ldh >= A + 1),
 * negative or non-finite weights.  No float atomics. */
int hsad_clone_value_tail(const float* heads, int ldh, const float* legal, const int64_t* action, const float* ret, const float* seq_len,
                          const float* weight, int T, int B, int A, float policy_weight, float value_weight, float* loss, float* vloss, int32_t* hits,
                          int32_t* decisions, int32_t* bad, int32_t* steps, void* dheads16, int ldo, void* stream);
/* hsad_clone_value_tail against a TARGET DISTRIBUTION per row instead of the one recorded move, one launch: target fp32 [M, A], a probability row
 * pi for every row m = t B + b (search values at a temperature, a teacher's policy; clone.soft_targets).  z, mx, S and softmax_j as there; with
 * sigma = sum_{legal j} pi_j in ascending j:  xent = sigma log S - sum_{legal j} pi_j (z_j - mx), the policy part of dheads16 column j < A is
 * policy_weight (sigma softmax_j - pi_j), summed in fp32 with the unchanged value term (which still reads action[m] and ret[m]) and rounded to
 * bf16 once.  hits and decisions are still counted against action[m].  A valid row is bad (counted in bad, all-zero gradient bits, no
 * contribution) when action[m] is bad by hsad_clone_tail's rule, a pi_j is negative or NaN, an illegal column has pi_j != 0 or
 * |sigma - 1| > 1e-3 -- a condition on the input, not a tolerance: a row made in fp32 from A <= 51 terms is within A 2^-23 of 1.  A single-legal
 * row must carry its mass on that action; it is xent = 0 and no policy gradient, as there.  Rows past seq_len read no target.  Where pi is the
 * one-hot of action[m] (1.0f and zeros) every output has the bits of hsad_clone_value_tail.  Refused: what hsad_clone_value_tail refuses, and
 * target == NULL (that call is hsad_clone_value_tail).  No float atomics, the same bits run to run.  The row is csrc/hsad_clone_soft.h. */
int hsad_clone_soft_tail(const float* heads, int ldh, const float* legal, const int64_t* action, const float* target, const float* ret,
                         const float* seq_len, const float* weight, int T, int B, int A, float policy_weight, float value_weight, float* loss,
                         float* vloss, int32_t* hits, int32_t* decisions, int32_t* bad, int32_t* steps, void* dheads16, int ldo, void* stream);
/* The loss of the learned hand belief, one launch.  Row m = t B + b; logits fp32 [T B, ldz], z[i 25 + type] for slot i; pool device
 * int64 [T, B], compat / cards device int32 [T, B, Hs] as hsad_env_hand_knowledge writes them (cards -1 = empty slot; the occupied
 * slots are the n before the first -1).  The belief factorises slot by slot with the exact belief as base measure; q = pool before
 * slot 0, rem = the slots after i, C as in hsad_env_hand_belief:
 *   w_i[type] = q[type] compat_i[type] C(rem, q - e_type)   (int64, exact);  F_i = the types with w_i != 0
 *   mx_i = max of z over F_i;  v = (float)w_i exp(z - mx_i);  S_i = sum of v over F_i, types ascending (fp32);  p_i = v (1 / S_i)
 *   then q[card_i] -= 1 with the true card of slot i.
 * Per valid row (t < seq_len[b]): nll = sum_i (log S_i - log (float)w_i[card_i]) - (z[card_i] - mx_i); nll0 = the same at z = 0 (the
 * score of the exact public belief); cards = the slots with |F_i| >= 2; hits / hits0 = of those, the slots where the true card is the
 * argmax of p_i / of w_i (lowest type on ties).  A row is bad -- counted in bad, nothing else, all-zero gradient bits -- when a true
 * card is outside F_i, a card id is outside 0..24 on an occupied slot, a card follows an empty slot, or an occupied slot has a
 * non-finite logit.  nll[b], nll0[b] float [B]: sums in ascending t; cards_n, hits, hits0, bad int32 [B].  dlogits16 (NULL = no
 * gradient): bf16 [T B, ldo], column i 25 + type = s (p_i[type] - [type == card_i]) on F_i with s = weight[b] / B, 0 elsewhere, for
 * empty slots and up to ldo; rows at or past seq_len are zero rows.  Zero logits give nll == nll0 bit for bit.  Refused
 * (HSAD_ERR_INVALID, nothing launched): a null argument, T or B < 1, Hs outside 1..5, ldz < 25 Hs, a gradient without weights or with
 * ldo < 25 Hs, T too long for one workgroup's step buffers.  No float atomics, the same bits run to run. */
int hsad_belief_tail(const float* logits, int ldz, const int64_t* pool, const int32_t* compat, const int32_t* cards, const float* seq_len,
                     const float* weight, int T, int B, int Hs, float* nll, float* nll0, int32_t* cards_n, int32_t* hits, int32_t* hits0, int32_t* bad,
                     void* dlogits16, int ldo, void* stream);
/* column sums (bias gradients) of a bf16 / fp32 [M, ld] matrix -> fp32 [N] */
int hsad_colsum(const void* src, int is_bf16, int M, int N, int ld, float* out, void* stream);
/* accumulating variant (no zeroing): out[col_map ? col_map[c] : c] += column sum c, and the same into out2 when given
 * (the two LSTM bias gradients are both the un-blocked column sums of dG) */
int hsad_colsum_acc(const void* src, int is_bf16, int M, int N, int ld, float* out, float* out2, const int32_t* col_map,
                    void* stream);
/* out[c] += column sum c without float atomics -- the same bits run to run: every 128-row block leaves its partial sums in `scratch`
 * (fp32 [ceil(M / 128)][N]), a second small launch adds them up in row-block order */
int hsad_colsum_acc_ordered(const void* src, int is_bf16, int M, int N, int ld, float* out, float* scratch, void* stream);
/* clip_grad_norm_(max_grad_norm) + Adam step over flat fp32 buffers (selfplay.py:231-235); step counts from 1;
 * scratch: fp32 [1]. */
int hsad_adam_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n, float max_grad_norm,
                   float lr, float beta1, float beta2, float eps, int step, float* scratch, void* stream);
/* The same followed by optim.zero_grad() (selfplay.py:234-235) in the same two launches: `grad` is left all zero, and no memset is
 * issued -- scratch2 is SIXTEEN floats, zeroed once by the caller; step k sums into slot k & 1 and clears the other one for step k + 1;
 * scratch2[4 + k % 12] receives the pre-clip global norm itself (clip_grad_norm_'s return value; a ring, so that a caller may read
 * it up to eleven steps late).
 * *grad_norm_sq (may be NULL) = the slot that holds this step's squared pre-clip norm (valid until step k + 2's kernel clears it). */
int hsad_adam_step_zero_grad(float* param, float* grad, float* exp_avg, float* exp_avg_sq, int64_t n, float max_grad_norm, float lr,
                             float beta1, float beta2, float eps, int step, float* scratch2, float** grad_norm_sq, void* stream);
/* R2D2Agent.act tail (r2d2.py:235-277): heads fp32 [N,ldh] (advantage in columns [0,A)), legal fp32 [N,A], eps fp32 [N]
 * (NULL = greedy) -> a, greedy_a int64 [N].  scratch fp32 [2 + ceil(N/256)].  Exploration draws come from a counter-based
 * hash of (seed, row, counter).  Every acting-tail entry point below computes its rows with ONE row function (as_tail_row / as_q_at of
 * csrc/hsad_act_sample.h, which states the arithmetic and its order): this one reads the rows from global memory (any row width);
 * hsad_act_select_q, _q2 and hsad_act_sample_q without temperatures are one kernel that stages them through LDS, called with fewer or
 * more of its optional arguments, so a row they share is the same bits by construction.  hsad_act_sample_q with temperatures runs the
 * same row written out in a kernel of its own (kept for its speed). */
int hsad_act_select(const float* heads, int ldh, const float* legal, const float* eps, int N, int A, uint64_t seed,
                    uint64_t counter, int64_t* a_out, int64_t* greedy_out, float* scratch, void* stream);
/* |reward + bootstrap * gamma^n * target_qa - online_qa| (R2D2Agent.compute_priority, r2d2.py:355-360), all fp32 [N] */
int hsad_nstep_priority(const float* qa, const float* target_qa, const float* reward, const float* bootstrap,
                        int multi_step, double gamma, int N, float* out, void* stream);
/* zero rows r of fp32 x[L,N,H] where flag[r / rows_per_flag] != 0 (hidden-state reset on terminal, r2d2_actor.h:109-126) */
int hsad_zero_rows(float* x, const uint8_t* flag, int L, int N, int H, int rows_per_flag, void* stream);
/* the same three results an acting step needs from the online heads in one pass: hsad_act_select + Q(s, a) of the chosen action
 * (hsad_q_head's value at a_out; qa_out may be NULL), and Q(s, action) alone for the target pass */
int hsad_act_select_q(const float* heads, int ldh, const float* legal, const float* eps, int N, int A, uint64_t seed,
                      uint64_t counter, int64_t* a_out, int64_t* greedy_out, float* qa_out, float* scratch, void* stream);
/* hsad_act_select_q for seats that play their softmax policy.  temp [N] (NULL = all 0): a row with temp[m] <= 0 is hsad_act_select_q's row
 * bit for bit (a, greedy, qa), and with temp == NULL the call is hsad_act_select_q.  On a row with temp[m] > 0 the exploration draw comes first (same hash, same uniform legal action when it
 * fires); otherwise a = an action sampled from softmax(adv_j / temp[m]) over the legal j -- at temp 1 the distribution whose
 * cross-entropy hsad_r2d2_clone_fwd minimises.  greedy_out is always hsad_act_select_q's; qa_out (optional) = hsad_q_at(heads, ..., a_out).
 * The sample uniform comes from the exploration hash of (seed, row, counter) by one more mixing round, or, with row_key int64 [N],
 * from (sample_seed, row_key[m]) alone: no row index and no counter, the caller owns uniqueness (and a row then plays the same wherever
 * it lies in the batch).  Draws, Pick and its fp32 range: csrc/hsad_act_sample.h.  scratch as hsad_act_select_q. */
int hsad_act_sample_q(const float* heads, int ldh, const float* legal, const float* eps, const float* temp, const int64_t* row_key,
                      uint64_t sample_seed, int N, int A, uint64_t seed, uint64_t counter, int64_t* a_out, int64_t* greedy_out,
                      float* qa_out, float* scratch, void* stream);
/* the same plus hsad_q_at(heads_target, greedy action) in ONE launch: the tail of hsad_r2d2_act when the two nets' heads come out of one
 * paired GEMM (Q_online(s, a) and Q_target(s, greedy) of r2d2.py:341-368 for the priorities); identical bits to the two calls */
int hsad_act_select_q2(const float* heads, const float* heads_target, int ldh, const float* legal, const float* eps, int N, int A,
                       uint64_t seed, uint64_t counter, int64_t* a_out, int64_t* greedy_out, float* qa_out, float* q_target_greedy,
                       float* scratch, void* stream);
int hsad_q_at(const float* heads, int ldh, const float* legal, const int64_t* action, int M, int A, float* qa, void* stream);
/* hsad_zero_rows for the whole carried state at once: fp32 h / c [L,N,H] and (optional) the bf16 copy of h */
int hsad_zero_state_rows(float* h, float* c, void* h_bf16, const uint8_t* flag, int L, int N, int H, int rows_per_flag, void* stream);
/* One recurrence of a multi-recurrence chunk launch (see hsad_lstm_forward_chunk for the field meanings) */
typedef struct hsad_lstm_fwd_rec {
  float* gates;
  const void* Whh_blocked;
  const void* h_prev16;
  const float* c_prev;
  void* hseq16;
  float* cseq;
  float* hT;  /* optional */
  void* xchg; /* optional bf16 scratch [Tc * 32*ceil(Bn/32) * H]: h tiles in hand-off order (contiguous 2 KB blocks) */
} hsad_lstm_fwd_rec;
typedef struct hsad_lstm_bwd_rec {
  const float* gates;
  const float* cseq;
  const float* c_before;
  const void* WhhT_blocked;
  const float* dO;
  void* dG16;
  float* dc_io;
  int has_next;
  void* xchg; /* optional bf16 scratch [Tc * 32*ceil(Bn/32) * 4H]: dG tiles in hand-off order */
  int saved_frag_major; /* gates / cseq / c_before are in the fragment-major order hsad_lstm_forward_fused stores (Bn % 32 == 0) */
  int tail_is_zero;     /* has_next == 0 only: dG16 slot Tc is known to hold zeros already (nothing ever writes it): skip its memset */
} hsad_lstm_bwd_rec;
/* nrec (<= 4 forward, <= 2 backward) independent recurrences of identical shape in ONE persistent launch, e.g. layer 0
 * on chunk c+1 next to layer 1 on chunk c, for the online and the target net at once.  The overlap is inside the launch,
 * so it does not depend on how HIP streams are multiplexed onto hardware queues.  Needs nrec * (H/32) * ceil(Bn/32)
 * co-resident workgroups (one per CU).  sync_scratch: uint32 [nrec*(Tc+2)*ceil(Bn/32) + 4]: one 64-bit XCD-placement word
 * per (recurrence, row block), the step counters, then the sticky timeout word.  Workgroups that exchange tiles are
 * mapped to block ids that share an XCD; a start-up handshake verifies it and only then uses the L2-local hand-off
 * (plain stores + L2 atomics), otherwise the cross-XCD protocol (write-through stores + device-scope atomics).
 * next_sync_scratch (may be NULL): ping-pong partner of the same size -- when given, sync_scratch must already be zero
 * (freshly zero-allocated, or zeroed by the previous launch of the pair) and this launch zeroes the partner instead of a
 * memset kernel in front of every launch. */
int hsad_lstm_forward_chunk_multi(int nrec, int Tc, int Bn, int H, const hsad_lstm_fwd_rec* recs, void* sync_scratch,
                                  void* next_sync_scratch, void* stream);
int hsad_lstm_backward_chunk_multi(int nrec, int Tc, int Bn, int H, const hsad_lstm_bwd_rec* recs, void* sync_scratch,
                                   void* next_sync_scratch, void* stream);
/* FUSED persistent forward (round 3): nnet independent nets x nlayer stacked LSTM layers over the whole sequence in ONE launch.
 * The input projection x_t W_ih^T is computed inside the recurrence: a workgroup's four waves split its 32 units, each keeps its
 * W_ih and W_hh slices as MFMA B fragments in registers for the whole sequence, the activation tiles arrive in LDS by LDS-DMA;
 * stacked layers run a step apart and read the bf16 h sequence of the layer below through the L2 of their shared XCD.  Replaces
 * the stand-alone projection GEMM + hsad_lstm_forward_chunk_multi stages of one nn.LSTM forward (pyhanabi/r2d2.py:99-105).
 * recs[net * nlayer + layer]; x16 == NULL (layer > 0 only): the input is hseq16 of the record before it.  Weights gate-blocked
 * (hsad_prepare_weight with the 32-unit permutation), bias = b_ih + b_hh in the same order; initial state zero; Bn a multiple of 32.
 * Outputs per record: hseq16 bf16 [T,Bn,H] row-major (also the hand-off buffer between workgroups), hT, and -- what BPTT reads,
 * NULL = not kept -- activated gates (T*Bn*4H floats) / cseq (T*Bn*H floats) in FRAGMENT-MAJOR order: gates
 * [T][Bn/32][H/32][wave 4][r 4][lane 64][i f g o], c [T][Bn/32][H/32][wave 4][lane 64][r 4], where (wave, lane, r) <-> row
 * 32 rb + 16 ((lane >> 3) & 1) + 4 (lane >> 4) + r, unit 32 nb + 8 wave + (lane & 7): the per-lane order of the fused recurrence
 * kernels, so every store (and every load of the BPTT recurrence) is a contiguous 1 KB per wave (hanabi_sad_amd/r2d2.py
 * unpack_saved_gates / unpack_saved_c restate the mapping for inspection).
 * Needs nlayer * (H/32) * ceil(nnet * Bn/32 / 8) <= CUs / 8 (a (net, row block)'s workgroups share an XCD), H in {256, 512}.
 * sync_scratch: uint32 [nnet*nlayer*(T+2)*Bn/32 + 4], ping-pong convention of hsad_lstm_forward_chunk_multi. */
typedef struct hsad_lstm_fused_rec {
  const void* Wih_blocked;
  const void* Whh_blocked;
  const float* bias_blocked;
  const void* x16;
  float* gates;
  float* cseq;
  void* hseq16;
  float* hT;
} hsad_lstm_fused_rec;
int hsad_lstm_forward_fused(int nnet, int nlayer, int T, int Bn, int H, const hsad_lstm_fused_rec* recs, void* sync_scratch,
                            void* next_sync_scratch, void* stream);
/* measurement hook (bench.py): HIP events around every hsad_lstm_forward_fused launch while enabled; _read returns the average
 * launch duration, the algorithmic FLOP per launch (2 T Bn 4H 2H per recurrence) and the launch count, synchronises, clears */
int hsad_lstm_fused_timing(int enable);
int hsad_lstm_fused_timing_read(double* avg_ms, double* avg_flop, int32_t* launches);
/* kind 0: the fused forward launches, 1: the fused BPTT launches (lstm_fused_bwd_kernel) recorded since the last read of that kind */
int hsad_lstm_fused_timing_read_kind(int kind, double* avg_ms, double* avg_flop, int32_t* launches);
/* FUSED persistent BPTT (round 3): the stacked layers of nnet nets over a chunk of Tc steps in ONE launch, one step apart; the gradient a
 * lower layer receives from the layer above, dO = dG_above W_ih_above (a stand-alone GEMM per chunk in hsad_lstm_backward_chunk_multi's
 * schedule), is computed inside the lower layer's recurrence from the hand-off tiles the layer above publishes (W_ih_above^T slice
 * register-resident, W_hh^T slice in LDS).  recs[net * nlayer + k], k = 0 the TOP layer of the launch (dO = the fp32 gradient from
 * outside, e.g. the heads), k > 0: WihT_above_blocked = the [H,4H] transposed gate-blocked W_ih of record k - 1's layer, dO NULL.
 * Other fields as hsad_lstm_bwd_rec (xchg required).  Needs nlayer * (H/32) * ceil(nnet * Bn/32 / 8) <= CUs / 8, H in {256, 512},
 * Bn % 32 == 0.  sync_scratch: uint32 [nnet*nlayer*(Tc+2)*Bn/32 + 4], ping-pong convention of hsad_lstm_forward_chunk_multi. */
typedef struct hsad_lstm_fused_bwd_rec {
  const void* WhhT_blocked;
  const void* WihT_above_blocked;
  const float* gates;
  const float* cseq;
  const float* c_before;
  const float* dO;
  void* dG16;
  float* dc_io;
  int has_next;
  void* xchg;
  int saved_frag_major;
  int tail_is_zero;
  void* xout;   /* split placement (NULL = off): a second hand-off buffer, laid out like xchg, on every record that feeds a layer below.
                 * The layers of a (net, row block) then run on DIFFERENT XCDs -- H/32 workgroups per XCD, half of a 32-CU XCD stays free
                 * for the weight-gradient GEMMs of the previous time chunk -- the feeding layer publishes its tile a second time, written
                 * through with an agent-scope counter; its own recurrence keeps the L2-local exchange.  Same bits either way.
                 * sync_scratch then holds uint32 [2 * nnet*nlayer*(Tc+2)*Bn/32 + 4]; grid = 8 * (H/32) * ceil(nnet*nlayer*Bn/32 / 8). */
  float* dO_stage;    /* split placement only (NULL = off), on a record WITH an X stream: fp32 [Tc, Bn, H].  The record's dO = dG^{l+1} W_ih^{l+1} is
                       * then computed by a projection stage of its own -- H/32 more workgroups per row block, a third pipeline stage between
                       * the two layers -- written here step by step, and the layer itself runs like a top layer whose dO arrives by counter:
                       * its step loses the X stream.  Give it for every record with an X stream or for none.  Sync scratch and timeout word
                       * are laid out for 2 * (records + projection stages). */
  /* sink stage (with projection stages only; on the LAST layer's record of every net, or of none): the gradient wrt the layer's input
   * sequence, dG W_ih (sink_WT = W_ih^T of THIS layer, blocked like WihT_above_blocked), as one more pipeline stage that writes bf16 rows
   * sink_out16 [Tc, Bn, H], zero where sink_mask16 [Tc, Bn, H] (bf16; NULL = no mask) is not > 0 -- the input-MLP backward GEMM with its
   * ReLU mask, off the tail of the update.  sink_xout: a hand-off buffer like xout for this layer's tiles. */
  const void* sink_WT;
  void* sink_out16;
  const void* sink_mask16;
  void* sink_xout;
  void* sink_outT16;       /* optional: write the sink's rows TRANSPOSED instead, bf16 [H][sink_ldT] (element (unit, t * Bn + row)); sink_out16 is */
  int sink_ldT;            /* then not written (pass any non-NULL pointer) */
  float* sink_bias_grad;   /* optional fp32 [H]: column sums of the (masked) rows over rows and steps are ADDED here */
  /* dGT16 (optional): the gradient wrt the gate pre-activations written TRANSPOSED, bf16 [4H][ldT] with element (gate-blocked column,
   * t * Bn + row) -- the A operand of the weight-gradient GEMMs, no transpose pass behind the launch -- INSTEAD of the row-major dG16
   * (which then only serves has_next; use with a single time chunk).  bias_grad0 / bias_grad1 (optional, fp32 [4H]): the column sums of dG
   * over all rows and steps are ADDED there at [bias_col_map[column]] (bias_col_map NULL = identity): the two LSTM bias gradients. */
  void* dGT16;
  int ldT;
  float *bias_grad0, *bias_grad1;
  const int32_t* bias_col_map;
  int layout_steps;   /* record 0 only; 0 = Tc.  Chunks of different lengths that share (ping-pong) sync blocks pass the LONGEST chunk length
                       * here: counters and the sticky timeout word then sit at the same place for every launch (read the timeout with
                       * that length), and a launch clears its partner block for any of them. */
  int wide_blocks;    /* record 0 only (round 6).  Non-zero: a launch of ONE two-layer net (nnet 1, nlayer 2, H 512) with projection + sink
                       * stages, fragment-major activations, dGT16 on both records, no has_next and Bn <= 128 runs the 16-row x 64-unit blocking
                       * (lstm_bptt_wide_kernel: weight slices in registers, 64 KB tiles, the four stages of a row block on one XCD).  xout /
                       * sink_xout then carry no tiles but are still REQUIRED (non-NULL) and WRITTEN: they are the scratch of the per-row-block
                       * bias partial sums, fp32 -- record 0's xout at least 8 * 4H floats, record 1's sink_xout at least 8 * 4H + 8 * H floats
                       * (buffers sized for tiles, Tc * Bn * 4H bf16, are larger than that for every Bn >= 32).  The row-major dG16 (slot Tc
                       * included) is not touched.  Same bits for dG, dO, d x.  0 = the 32 x 32 blocking (A/B); other shapes ignore it. */
} hsad_lstm_fused_bwd_rec;
int hsad_lstm_backward_fused(int nnet, int nlayer, int Tc, int Bn, int H, const hsad_lstm_fused_bwd_rec* recs, void* sync_scratch,
                             void* next_sync_scratch, void* stream);
/* Chunked persistent recurrences for layer pipelining (one launch per chunk of Tc steps, state carried across
 * launches): h_prev16 bf16 [Bn,H] / c_prev fp32 [Bn,H] = state entering the chunk (c_prev NULL = zeros). */
int hsad_lstm_forward_chunk(int Tc, int Bn, int H, float* gates, const void* Whh_blocked, const void* h_prev16,
                            const float* c_prev, void* hseq16, float* cseq, float* hT, void* sync_scratch, void* stream);
/* all sequence pointers address the chunk's first step; dG16 slot Tc = gradient of the following chunk's first step
 * (has_next) or scratch that is zeroed; c_before = c of the step before the chunk (NULL = zeros); dc_io fp32 [Bn,H]
 * carries dc between chunks (caller zeroes it before the last-in-time chunk). */
int hsad_lstm_backward_chunk(int Tc, int Bn, int H, const float* gates, const float* cseq, const float* c_before,
                             const void* WhhT_blocked, const float* dO, void* dG16, float* dc_io, int has_next,
                             void* sync_scratch, void* stream);

/* ------------------------------------------------------------------------------------------
 * COMPOSITE entry points (csrc/hsad_agent.hip, the learner in csrc/hsad_learner.hip): the agent methods the reference's native side calls through
 * rela::BatchRunner -- `act`, `compute_priority` (rela/batch_runner.h:74-113, rela/r2d2_actor.h:61-172 ->
 * pyhanabi/r2d2.py:247-361) -- and the learner step of pyhanabi/selfplay.py:208-244 (R2D2Agent.loss r2d2.py:383-499, backward,
 * clip_grad_norm_, Adam, sync_target_with_online), each as ONE call on plain pointers.  The library owns the weights (one flat
 * fp32 vector per net: tensors back to back in the order of hsad_r2d2_param_name = the reference's state_dict names), their bf16
 * kernel operands and all workspace; a C++ / pybind host needs nothing else to run the agent and the learner.
 * ------------------------------------------------------------------------------------------ */
typedef struct hsad_r2d2_net hsad_r2d2_net;
typedef struct hsad_r2d2_learner hsad_r2d2_learner;
/* R2D2Net(in_dim, hid_dim, out_dim = num_action, 2 LSTM layers, hand_size) (pyhanabi/r2d2.py:22-57).  with_backward = 1: the
 * learner's online net (keeps transposed operands; never steps single rows), 0: acting / target nets. */
int hsad_r2d2_net_create(int in_dim, int hid_dim, int num_action, int hand_size, int with_backward, int device, hsad_r2d2_net** out);
/* The general R2D2Net(…, num_lstm_layer, hand_size, num_fc_layer, skip_connect) (pyhanabi/r2d2.py:22-57): num_fc_layer 1..2 (net.0 /
 * net.2), num_lstm_layer 1..3 (--num_lstm_layer, selfplay.py:50), skip_connect = `o + x` in R2D2Net.act ONLY (r2d2.py:74-75;
 * R2D2Net.forward -- compute_priority, td_error, the learner -- ignores it in the reference, and so does this library).  The
 * Other-Play zoo models M3..M11 (pyhanabi/utils.py:46-57) are (1 fc, skip), (2 fc), (2 fc, skip).  hsad_r2d2_net_create = (1, 2, 0).
 * Parameter tensors: hsad_r2d2_net_num_params / _param_name (state_dict names; the flat vector holds them in that order). */
int hsad_r2d2_net_create_ex(int in_dim, int hid_dim, int num_action, int hand_size, int num_fc_layer, int num_lstm_layer, int skip_connect,
                            int with_backward, int device, hsad_r2d2_net** out);
int hsad_r2d2_net_num_params(const hsad_r2d2_net* net);
const char* hsad_r2d2_net_param_name(const hsad_r2d2_net* net, int i);
int hsad_r2d2_net_arch(const hsad_r2d2_net* net, int32_t* num_fc_layer, int32_t* num_lstm_layer, int32_t* skip_connect);
void hsad_r2d2_net_destroy(hsad_r2d2_net* net);
int hsad_r2d2_num_params(void);                 /* 16 tensors */
const char* hsad_r2d2_param_name(int i);        /* "net.0.weight", ..., "pred.bias" */
int64_t hsad_r2d2_net_param_count(const hsad_r2d2_net* net);          /* fp32 elements of the flat vector */
int64_t hsad_r2d2_net_param_offset(const hsad_r2d2_net* net, int i);  /* element offset of tensor i (i = 16: the end) */
int64_t hsad_r2d2_net_param_size(const hsad_r2d2_net* net, int i);
float* hsad_r2d2_net_params(hsad_r2d2_net* net);                      /* device pointer: write weights here, then refresh */
int hsad_r2d2_net_refresh(hsad_r2d2_net* net, void* stream);          /* re-derive the bf16 / permuted / transposed operands */
uint64_t hsad_r2d2_net_version(const hsad_r2d2_net* net);             /* bumped by every refresh */
int hsad_r2d2_net_in_dim_padded(const hsad_r2d2_net* net);            /* row length of a bf16 observation operand (in_dim rounded up to 64) */
/* R2D2Agent.act for N rows (one per (game, player)): priv_s fp32 [N,F] -- or priv_s_bf16 [N, in_dim_padded] zero-padded, as
 * hsad_env_bind_packed writes it (then priv_s may be NULL and no cast pass runs) --, legal_move [N,A], eps [N] (NULL = greedy), hidden state
 * h0 / c0 fp32 [L,N,H] in, h_out / c_out out (h0_bf16 / h_out_bf16, optional: the bf16 copy the fused cell kernels read / write
 * anyway, carried by the caller to save a cast per step) -> a, greedy_a int64 [N].  q_online_a / q_target_greedy (optional; the
 * latter needs the former and `target`): Q_online(s, a) of the pass that picked the action and Q_target(s, greedy_a) from one target-net pass, i.e. what
 * compute_priority needs from this step.  Exploration: counter-based hash of (seed, row, counter). */
int hsad_r2d2_act(hsad_r2d2_net* online, hsad_r2d2_net* target, int N, const float* priv_s, const void* priv_s_bf16,
                  const float* legal_move, const float* eps, const float* h0, const float* c0, const void* h0_bf16, uint64_t seed, uint64_t counter,
                  int64_t* a, int64_t* greedy_a, float* h_out, float* c_out, void* h_out_bf16, float* q_online_a,
                  float* q_target_greedy, void* stream);
/* hsad_r2d2_act's single-net path (target = NULL) with hsad_act_sample_q as its tail: temp [N], row_key int64 [N] and sample_seed as
 * there.  With temp == NULL every output equals hsad_r2d2_act(net, NULL, ...) bit for bit; h_out / c_out never depend on temp.
 * q_online_a (optional) = Q_net(s, a) at the action taken; refused on a skip_connect net like hsad_r2d2_act's. */
int hsad_r2d2_act_soft(hsad_r2d2_net* net, int N, const float* priv_s, const void* priv_s_bf16, const float* legal_move, const float* eps,
                       const float* temp, const int64_t* row_key, uint64_t sample_seed, const float* h0, const float* c0,
                       const void* h0_bf16, uint64_t seed, uint64_t counter, int64_t* a, int64_t* greedy_a, float* h_out, float* c_out,
                       void* h_out_bf16, float* q_online_a, void* stream);
/* the two halves of that call separately: hsad_r2d2_act with target = NULL, q_target_greedy = NULL and q_online_a set gives the action,
 * the greedy action, the new state and Q_online(s, a); hsad_r2d2_target_q gives Q_target(s, greedy_a) from the same inputs.  A caller
 * that issues the env step between them (it only needs the actions) can run it next to the target pass. */
int hsad_r2d2_target_q(hsad_r2d2_net* target, int N, const float* priv_s, const void* priv_s_bf16, const float* legal_move,
                       const float* h0, const float* c0, const void* h0_bf16, const int64_t* greedy_a, float* q_target_greedy, void* stream);
/* R2D2Agent.compute_priority (r2d2.py:305-361): |r + bootstrap gamma^n Q_target(s', argmax adv_online(s')) - Q_online(s, a)|.
 * num_player > 1 = VDN: Q summed over the players of a game; reward / bootstrap / priority are then per game [N / num_player].
 * next_greedy_a (may be NULL): the argmax when the caller already has it (the act() of the same iteration). */
int hsad_r2d2_compute_priority(hsad_r2d2_net* online, hsad_r2d2_net* target, int N, int num_player, const float* priv_s,
                               const float* legal_move, const int64_t* a, const float* next_priv_s, const float* next_legal_move,
                               const float* h0, const float* c0, const float* next_h0, const float* next_c0, const float* reward,
                               const float* bootstrap, int multi_step, double gamma, const int64_t* next_greedy_a, float* priority,
                               void* stream);
/* Q_net(s, action) fp32 [N] for one step from the carried hidden state: the single pass compute_priority is built from (an actor
 * redoes Q_online(s_{t-n}, a_{t-n}) with it when the weights were synced inside the n-step window) */
int hsad_r2d2_q_of(hsad_r2d2_net* net, int N, const float* priv_s, const float* legal_move, const int64_t* action, const float* h0,
                   const float* c0, float* qa, void* stream);
/* learner over batches of T steps x rows_per_step rows (rows = batch size, x num_player for VDN); nets stay owned by the caller */
int hsad_r2d2_learner_create(hsad_r2d2_net* online, hsad_r2d2_net* target, int T, int rows_per_step, int multi_step, double gamma,
                             float lr, float eps, float grad_clip, hsad_r2d2_learner** out);
void hsad_r2d2_learner_destroy(hsad_r2d2_learner* learner);
int hsad_r2d2_learner_set_schedule(hsad_r2d2_learner* learner, int chunks, int wgrad_split);
/* Recurrence schedule of a learner: THE table of the flag word (the default is 0x39 | 1 << 8 = bits 0, 3, 4, 5 with one BPTT chunk).  The
 * flags say what is asked for; what a shape cannot hold falls back to off (bits 3 / 4 / 5: their 16-workgroup groups -- 2 / 3 / 4 per 32-row
 * block -- must fit the chip) and hsad_r2d2_learner_plan reports what ran.  Synchronises.
 *   bit 0      the forward recurrences of hsad_r2d2_loss_fwd run as whole-sequence fused launches (hsad_lstm_forward_fused: projection inside
 *              the recurrence, layers one step apart, online + target net together) and BPTT as hsad_lstm_backward_fused launches (both layers,
 *              dO of the lower layer inside its recurrence) when the shape allows (H in {256, 512}, rows % 32 == 0, a (net, row block)'s
 *              workgroups fit an XCD); 0: the chunk-pipelined schedule of rounds 1-2 (stand-alone projection / dO GEMMs between chunk launches)
 *   bit 1      with bit 0: keep the chunk-pipelined BPTT (A/B of the backward schedule)
 *   bit 2      hsad_r2d2_optimizer_step re-derives the LSTM matrices (95 % of the operand bytes) on the learner's side stream, next to the
 *              following update's input layer; every entry point that reads a net's LSTM operands waits for that half first (an event, no
 *              host synchronisation).  Off by default: measured 1.521 against 1.504 ms per update with everything in line
 *   bit 3      split placement of the fused BPTT (hsad_lstm_fused_bwd_rec.xout): the two layers of a row block on different XCDs, half of
 *              every XCD free for the chunk-wise weight gradients on the side stream; meant for bits 8-15 >= 2
 *   bit 4      with bit 3: the lower layer's dO = dG1 W_ih1 in a projection stage of its own (hsad_lstm_fused_bwd_rec.dO_stage)
 *   bit 5      with bits 3, 4: the input layer's d x = dG0 W_ih0 (ReLU-masked) as a sink stage of the BPTT launch
 *   bit 6      the single-chunk fused BPTT leaves dG row-major and two transpose passes (+ bias column sums) follow it, as in every
 *              chunked schedule; 0 (default, needs the sink stage): the launch writes dG transposed and adds the bias gradients itself
 *   bit 7      off: the four LSTM weight gradients and the input layer's of a single-chunk fused BPTT as six split-K GEMMs on two streams
 *              (round 4) instead of one grouped launch of the 256 x 256 core + one slab pass (hsad_gemm_nt_bf16_group_splitk; one fc layer)
 *   bits 8-15  time chunks of the fused BPTT, 1..8 (the weight gradients are added up per chunk); 0 keeps the current setting
 *   bits 16-23 fused BPTT in TWO unequal chunks: steps [n, T) first, the head [0, n) last (0 = equal chunks per bits 8-15) -- the long
 *              chunk's weight gradients run next to the head's recurrence, only the head's are left for the end of the update
 *   bit 24     off: the chain between the two recurrences as four launches (head GEMM pair, hsad_q_head, loss tail, dO GEMM) instead of two (both
 *              nets' heads + the online dueling head in one launch; the loss tail forming d loss / d o itself) -- identical bits, A/B
 *   bit 25     off: the 32 x 32 blocking of the four-stage single-chunk BPTT launch instead of the 16-row x 64-unit one
 *              (lstm_bptt_wide_kernel, taken where the shape allows) -- A/B */
int hsad_r2d2_learner_set_fused(hsad_r2d2_learner* learner, int fused_fwd);
/* What the last hsad_r2d2_loss_fwd ran and -- as the hsad_r2d2_loss_bwd behind it resolved it, else as it would be under the current flags --
 * its backward half: the schedule the flags and the shape resolve to (HSAD_ERR_STATE before the first loss_fwd).  Kinds: 0 plain (per layer a
 * projection GEMM + an unchunked recurrence), 1 chunk-pipelined, 2 fused.  Reports, changes nothing. */
typedef struct hsad_learner_plan {
  int32_t fwd_kind, fwd_nets, fwd_layers;   /* fused forward: nets and stacked layers per launch (else 0) */
  int32_t fwd_chunks;                       /* time chunks of the chunk-pipelined schedule */
  int32_t bwd_kind, bptt_chunks;
  int32_t split, proj, sink;                /* fused BPTT: stages that were asked for and fit the chip */
  int32_t dgt_in_kernel, group;             /* ... dG transposed + bias gradients inside the launch; one grouped weight-gradient launch */
  int32_t wide_requested;                   /* ... the 16-row x 64-unit blocking was asked of the launcher (it takes it at H = 512, rows <= 128) */
  int32_t chunk_input;                      /* chunked fused BPTT: the input layer's backward pass per chunk on the side stream */
  int32_t one_launch_heads, dO_in_loss_tail;
} hsad_learner_plan;
int hsad_r2d2_learner_plan(const hsad_r2d2_learner* learner, hsad_learner_plan* out);
float* hsad_r2d2_learner_grad(hsad_r2d2_learner* learner);            /* flat gradient, same layout as the net's parameters */
int hsad_r2d2_learner_timed_out(hsad_r2d2_learner* learner, int32_t* timed_out);
/* hsad_r2d2_loss_bwd with importance weights that arrive after the forward pass (the torch.autograd face of R2D2Agent.loss: the reference's
 * driver multiplies by the weights after agent.loss() returned, pyhanabi/selfplay.py:226-228): weight_b = B x d objective / d loss_b */
int hsad_r2d2_loss_bwd_weighted(hsad_r2d2_learner* learner, const float* weight, const float* seq_len, void* stream);
/* learning rate / Adam epsilon / clipping norm (<= 0: none) of hsad_r2d2_optimizer_step */
int hsad_r2d2_learner_set_optim(hsad_r2d2_learner* learner, float lr, float eps, float max_grad_norm);
/* (hsad_r2d2_loss_fwd / _loss_bwd / _optimizer_step fail with HSAD_ERR_STATE by themselves once an EARLIER update's persistent recurrence
 * has given up waiting for a sibling workgroup: every update reports its sticky words to a pinned host word, looked at without a
 * synchronisation.)  Test hook: set / clear such a word as a timed-out launch would. */
int hsad_r2d2_learner_inject_timeout(hsad_r2d2_learner* learner, int set);
/* R2D2Agent.loss forward: priv_s [T,rows,F], legal_move [T,rows,A], a int64 [T,rows], own_hand [T,rows,3*hand] (NULL without the
 * aux task); reward / bootstrap [T,B], seq_len / weight [B] with B = rows / num_player games -> loss [B], priority [T,B].
 * want_grad keeps what loss_bwd needs (weight required).  priv_s_bf16 (instead of priv_s): [T*rows, in_dim_padded] zero-padded bf16,
 * e.g. what hsad_replay_sample writes for an HSAD_BITS field set to HSAD_BITS_AS_BF16; no cast pass, and it must stay valid until
 * loss_bwd has been issued. */
int hsad_r2d2_loss_fwd(hsad_r2d2_learner* learner, const float* priv_s, const void* priv_s_bf16, const float* legal_move, const int64_t* a, const float* reward,
                       const float* bootstrap, const float* seq_len, const float* own_hand, const float* weight, int num_player,
                       float pred_weight, float* loss, float* priority, int want_grad, void* stream);
/* (loss * weight).mean().backward(): BPTT into hsad_r2d2_learner_grad; the batch given to loss_fwd must still be alive */
int hsad_r2d2_loss_bwd(hsad_r2d2_learner* learner, void* stream);
/* Behaviour cloning: the forward half of a supervised update on recorded moves.  IQL layout (rows = sequences, no num_player); runs the ONLINE
 * net only, on the schedule the planner resolves for one net (hsad_learner_plan.fwd_nets == 1 where fused), then hsad_clone_tail: loss [rows],
 * hits / decisions / bad int32 [rows].  want_grad (weight required) leaves d mean_b(weight_b loss_b) / d heads for the unchanged
 * hsad_r2d2_loss_bwd and hsad_r2d2_optimizer_step; hsad_r2d2_loss_bwd_weighted behind it is refused (HSAD_ERR_STATE).  No auxiliary task. */
int hsad_r2d2_clone_fwd(hsad_r2d2_learner* learner, const float* priv_s, const void* priv_s_bf16, const float* legal_move, const int64_t* a,
                        const float* seq_len, const float* weight, float* loss, int32_t* hits, int32_t* decisions, int32_t* bad, int want_grad,
                        void* stream);
/* hsad_r2d2_clone_fwd with hsad_clone_value_tail at its end: the same path (online net only, the one-net schedule, the same hand-off to
 * hsad_r2d2_loss_bwd + hsad_r2d2_optimizer_step; hsad_r2d2_loss_bwd_weighted behind it is refused), and additionally Q(o_t, a_t) of the online net
 * is fitted to ret [T, rows], the return-to-go of the recorded game: vloss [rows] = the Huber sums, steps int32 [rows] = the rows they run over.
 * The objective is mean_b(weight_b (policy_weight loss_b + value_weight vloss_b)); the value head now gets a gradient.  value_weight == 0:
 * ret and vloss may be NULL.  Negative or non-finite weights are refused before anything is launched. */
int hsad_r2d2_clone_value_fwd(hsad_r2d2_learner* learner, const float* priv_s, const void* priv_s_bf16, const float* legal_move, const int64_t* a,
                              const float* ret, const float* seq_len, const float* weight, float policy_weight, float value_weight, float* loss,
                              float* vloss, int32_t* hits, int32_t* decisions, int32_t* bad, int32_t* steps, int want_grad, void* stream);
/* hsad_r2d2_clone_value_fwd with hsad_clone_soft_tail at its end: target [T, rows, A], a probability row per (step, sequence), takes the place
 * of the one-hot of a in the cross-entropy (a is still what hits / decisions count against and what the value term reads).  The same one-net
 * schedule, the same hand-off to hsad_r2d2_loss_bwd + hsad_r2d2_optimizer_step, hsad_r2d2_loss_bwd_weighted behind it is refused, and every
 * argument is checked before anything is launched (target == NULL included).  Distillation of a search into its blueprint is this call on
 * clone.soft_targets of the search's action values. */
int hsad_r2d2_clone_soft_fwd(hsad_r2d2_learner* learner, const float* priv_s, const void* priv_s_bf16, const float* legal_move, const int64_t* a,
                             const float* target, const float* ret, const float* seq_len, const float* weight, float policy_weight,
                             float value_weight, float* loss, float* vloss, int32_t* hits, int32_t* decisions, int32_t* bad, int32_t* steps,
                             int want_grad, void* stream);
/* clip_grad_norm_ + Adam.step + operand refresh; grad_norm_sq_dev (may be NULL) receives a device pointer to the squared
 * pre-clip gradient norm */
int hsad_r2d2_optimizer_step(hsad_r2d2_learner* learner, float beta1, float beta2, float** grad_norm_sq_dev, void* stream);
/* device float: the pre-clip global gradient norm of the last hsad_r2d2_optimizer_step (what clip_grad_norm_ returns, selfplay.py:231);
 * the location stays untouched for the next eleven steps */
const float* hsad_r2d2_learner_grad_norm_dev(const hsad_r2d2_learner* L);
int hsad_r2d2_sync_target_with_online(hsad_r2d2_learner* learner, void* stream);

/* ------------------------------------------------------------------------------------------
 * Multi-GPU exchange (csrc/hsad_comm.hip): one process per GPU, RCCL over xGMI, bound at run time (dlopen) -- what
 * hanabi_sad_amd/dist.py ReplayLink does through torch.distributed, for a host that is not Python.  Stream-ordered, no host
 * synchronisation.  The host distributes the unique id (its own rendezvous: a file, a socket, MPI ...).
 *   reference: BatchRunner::updateModel across devices (rela/batch_runner.h:74-77), PrioritizedReplay::sample /
 *   updatePriority over every actor's data (rela/prioritized_replay.h:208-257).
 * ------------------------------------------------------------------------------------------ */
typedef struct hsad_comm hsad_comm;
int hsad_comm_unique_id(void* out, int out_bytes);           /* >= 128 bytes; rank 0 creates it, every rank passes the same bytes */
int hsad_comm_init(const void* unique_id, int rank, int world, int device, hsad_comm** out);
void hsad_comm_destroy(hsad_comm* comm);
int hsad_comm_rank(const hsad_comm* comm);
int hsad_comm_world(const hsad_comm* comm);
/* parameters as ONE flat bucket (hsad_r2d2_net_params of the learner's net on root, of the acting nets elsewhere; refresh after) */
int hsad_comm_bcast_params(hsad_comm* comm, float* params, int64_t count, int root, void* stream);
/* one prioritized draw over the concatenation of all ranks' shards: statistics all-gather (16 bytes per rank), hsad_replay_serve
 * on every shard, then every rank's wire buffer [batch][hsad_replay_wire_bytes] to root in one grouped send / recv.  canon [batch]:
 * the same uniforms on every rank (root's, e.g. sent along by hsad_comm_bcast_params' sibling call or a header broadcast).
 * root then calls hsad_replay_assemble(shard, batch, world, wire_all, owner_out, ...).  wire_all: root only, [world][batch][bytes]. */
int hsad_comm_gather_batch(hsad_comm* comm, hsad_replay* shard, int batch, const float* canon, int root, int32_t* owner_out,
                           uint8_t* wire_mine, uint8_t* wire_all, void* stream);
/* new priorities [batch] of the oldest outstanding draw (root's pointer; NULL elsewhere) + that draw's owner[]: broadcast, and every
 * shard writes back the positions it owned (hsad_replay_update_owned) */
int hsad_comm_scatter_priority(hsad_comm* comm, hsad_replay* shard, int batch, const float* priority, const int32_t* owner, int root,
                               void* stream);
/* ONE point-to-point ("star") round, the shape hanabi_sad_amd/dist.py ReplayLink runs by default: every message is between root (the
 * learner) and one other rank, so no actor waits for another actor's statistics or rows.
 *   hdr     device float32 [2 * batch + 4 * world]: canonical uniforms | priorities of the oldest outstanding draw | (sum, size) of
 *           every shard as float64 pairs.  root fills the first two parts; the library fills the third with what the replies of the
 *           PREVIOUS round reported (HSAD_LINK_PRIME, the first round: collected up front) and sends the whole header to every rank.
 *   flags   HSAD_LINK_* ; the same value on every rank (the host's own signalling: dist.py uses the rendezvous store).
 *   answer_owner   owner[] of the draw the priorities belong to (HSAD_LINK_HAS_PRIO; each rank keeps its owner_out of earlier rounds).
 *   every rank serves from the header's statistics (hsad_replay_serve stretches its share onto the shard's present weight sum and
 *   scales the raw weights), THEN writes the late priorities back, so hsad_replay_set_outstanding needs one draw more than rounds
 *   are pipelined.  root: wire_all [world][batch][bytes] is ready for hsad_replay_assemble, hsad_comm_all_stats = what the draw was
 *   cut with.  HSAD_LINK_PARAMS: params [param_count] leave root for every rank behind the rows.
 *   reference: PrioritizedReplay::sample / updatePriority (rela/prioritized_replay.h:208-257), BatchRunner::updateModel
 *   (rela/batch_runner.h:74-77) across processes. */
#define HSAD_LINK_PARAMS 1
#define HSAD_LINK_STOP 2
#define HSAD_LINK_HAS_PRIO 4
#define HSAD_LINK_PRIME 8
int hsad_comm_star_round(hsad_comm* comm, hsad_replay* shard, int batch, float* hdr, int flags, int root, const int32_t* answer_owner,
                         int32_t* owner_out, uint8_t* wire_mine, uint8_t* wire_all, float* params, int64_t param_count, void* stream);
/* The same round in two halves, so that rounds OVERLAP: the learner opens a round `ahead` updates before it trains on its batch (the
 * reference's sampler prefetches like that: rela/prioritized_replay.h:229-237, pyhanabi/selfplay.py prefetch = 3).  The root drives two
 * communicators -- `down` for headers and parameters, `up` for rows and statistics -- on two streams (on one communicator the header of
 * round r + 1 would queue behind the receive of round r's replies) and a ring of per-round buffers (hdr, owner_out, wire_all,
 * stats_reply); hsad_replay_set_outstanding(ahead + 2).
 *   hsad_comm_star_open     root: statistics (stats_known: the stats_reply of the newest round the host has collected; HSAD_LINK_PRIME:
 *                           collected into stats_prime first) -> header tail, header (and parameters) to every rank on `down`
 *   hsad_comm_star_collect  root, right behind it: receives posted on `up`, own shard served, its statistics into stats_reply[root];
 *                           when stream_up has passed this call, wire_all is ready for hsad_replay_assemble
 *   hsad_comm_star_serve    every other rank, on its own stream: [PRIME: statistics up] header in (down) -> serve -> late priorities ->
 *                           rows + statistics up -> [PARAMS: parameters in (down)] */
int hsad_comm_star_open(hsad_comm* down, hsad_comm* up, hsad_replay* shard, int batch, float* hdr, int flags, const double* stats_known,
                        double* stats_prime, float* params, int64_t param_count, void* stream_down, void* stream_up);
int hsad_comm_star_collect(hsad_comm* down, hsad_comm* up, hsad_replay* shard, int batch, float* hdr, int flags, const int32_t* answer_owner,
                           int32_t* owner_out, uint8_t* wire_all, double* stats_reply, void* stream_down, void* stream_up);
int hsad_comm_star_serve(hsad_comm* down, hsad_comm* up, hsad_replay* shard, int batch, float* hdr, int flags, int root,
                         const int32_t* answer_owner, int32_t* owner_out, uint8_t* wire_mine, float* params, int64_t param_count, void* stream);
const double* hsad_comm_all_stats(const hsad_comm* comm);   /* device [world][2] (sum, size) of the last gather: the importance weights' N and sum */

/* ------------------------------------------------------------------------------------------
 * fp32-EXACT mode of the R2D2 network (csrc/hsad_r2d2_f32.hip): the reference's arithmetic type throughout
 * (pyhanabi/r2d2.py:42-57,99-131,383-499) on v_mfma_f32_32x32x2_f32 (bitwise a k-ordered fmaf chain) with libm-accurate
 * activations -- the mode the golden vectors are matched in at fp32 round-off, and the yardstick the bf16 path's stated
 * tolerances are measured against.  Correctness mode: one launch per time step, no reduced-precision storage.
 * ------------------------------------------------------------------------------------------ */
/* C[M,N] = A * B^T (+bias[N]) (ReLU) (zero where relu_mask <= 0) (accumulated into C); operand element (m,k) of A at
 * A[m*sam + k*sak], (n,k) of B at B[n*sbn + k*sbk] -- any of NT / NN / TN / TT without materialised transposes;
 * row_map (may be NULL): result row r lands in row row_map[r] of C. */
int hsad_gemm_f32(const float* A, int64_t sam, int64_t sak, const float* B, int64_t sbn, int64_t sbk, int M, int N, int K,
                  const float* bias, float* C, int ldc, int relu, int accumulate, const float* relu_mask, int ldmask,
                  const int32_t* row_map, void* stream);
/* nn.LSTM cell (gate columns [i|f|g|o] x H, natural order): gates [Bn,4H] in = pre-activations, out = activated gates;
 * c_prev (NULL = zeros) -> c_out, h_out [Bn,H]. */
int hsad_lstm_cell_f32_forward(float* gates, const float* c_prev, float* c_out, float* h_out, int Bn, int H, void* stream);
/* BPTT through one cell: dh = dO (may be NULL) + dh_rec (may be NULL); dc_io [Bn,H] carries dc (in: from step t+1, out:
 * for step t-1); dG [Bn,4H] = gradient wrt the gate pre-activations. */
int hsad_lstm_cell_f32_backward(const float* gates, const float* c, const float* c_prev, const float* dO, const float* dh_rec,
                                float* dc_io, float* dG, int Bn, int H, void* stream);
/* out[i] = a[i] * b[i], n elements, bf16 (is_bf16) or fp32: the private x public gating of the OBL model family
 * (pyhanabi/tools/obl_model.py:96-99) */
int hsad_eltwise_mul(const void* a, const void* b, void* out, int64_t n, int is_bf16, void* stream);
/* hsad_heads_backward with an fp32 output [M, ldo] */
int hsad_heads_backward_f32(const float* dqa, const float* legal, const int64_t* action, const float* heads, int ldh,
                            const float* own_hand, const float* weight, int M, int B, int A, int NP, float pred_scale,
                            float* out32, int ldo, void* stream);

/* ------------------------------------------------------------------------------------------
 * ACTOR LOOP BODY (csrc/hsad_actor.hip): one iteration of HanabiThreadLoop::mainLoop (cpp/thread_loop.h:42-88) with
 * R2D2Actor::act / postAct (rela/r2d2_actor.h:61-172) for ALL games of an env object, as ONE call: reset the games that ended ->
 * act (hsad_r2d2_act with cached Q-values) -> push observation + action -> env step -> push reward / terminal -> zero the carried
 * state of ended games -> pop the transition that left the n-step window -> priority from the cached Q-values (the online pass on
 * s_{t-n} redone if the weights were synced in between) -> sequence push -> flush finished sequences into the replay.  The library
 * owns the carried hidden state, the Q-value ring, the sequence writer and the side streams (reset and flush overlap the rest);
 * env, nets, replay and the env's output buffers belong to the caller.  IQL (one transition per (game, player)) and VDN (one per
 * game) layouts of the reference's create.py:98-131.  Needs the packed env outputs (hsad_env_bind_packed, keep_float32_obs = 0 is
 * fine) and a replay created with the transition layout below.
 * ------------------------------------------------------------------------------------------ */
typedef struct hsad_actor hsad_actor;
typedef struct hsad_actor_config {
  int32_t vdn;         /* 1: one transition per game with the players' rows concatenated; 0: one per (game, player) */
  int32_t multi_step;  /* n of the n-step return */
  int32_t seq_len;     /* R2D2Buffer length (--max_len) */
  int32_t hand_size;
  int32_t hid_dim;
  float gamma;
  float eta;           /* aggregatePriority */
  uint64_t seed;       /* eps-greedy stream (hsad_r2d2_act) */
} hsad_actor_config;
/* what the caller bound to the env (hsad_env_bind_outputs / hsad_env_bind_packed); layout of the transition fields the replay must
 * have been created with: priv_s BITS(m*F), legal_move BITS(m*A), eps F32(m), own_hand BITS(m*3*hand), a I64(m), greedy_a I64(m),
 * m = players (VDN) or 1 (IQL), bit fields in m segments */
typedef struct hsad_actor_io {
  const float* legal_move;
  const float* own_hand;
  const float* eps;
  const float* reward;
  const uint8_t* terminal;
  const uint64_t* priv_bits;
  const uint64_t* legal_bits;
  const uint64_t* own_bits;
  const void* priv_s_bf16;   /* [G*P, hsad_r2d2_net_in_dim_padded(online)] */
} hsad_actor_io;
int hsad_actor_create(hsad_env* env, hsad_r2d2_net* online, hsad_r2d2_net* target, hsad_replay* replay, const hsad_actor_config* cfg,
                      const hsad_actor_io* io, hsad_actor** out);
void hsad_actor_destroy(hsad_actor* actor);
/* one iteration for every game; everything is enqueued on `stream` and the actor's two side streams, the host never waits
 * (unless hsad_actor_set_run_ahead bounds it) */
int hsad_actor_step(hsad_actor* actor, void* stream);
/* steps (0 = unbounded, the default; 1..7) the host may be ahead of the device: hsad_actor_step then waits, polling an event, until
 * step t - steps has left the device.  An actor rank of a multi-GPU job sets 2-3: whatever is stream-ordered behind its steps -- the
 * learner's sampling round (rela/prioritized_replay.h:208-257 across processes), new parameters (batch_runner.h:74-77) -- is at most
 * that many steps away, and the device still never runs dry. */
int hsad_actor_set_run_ahead(hsad_actor* actor, int steps);
int64_t hsad_actor_num_act(const hsad_actor* actor);        /* R2D2Actor::numAct summed over the per-player actors */
int64_t hsad_actor_num_redo(const hsad_actor* actor);       /* steps whose Q_online(s_{t-n}, a) pass was redone after a weight sync */
const int32_t* hsad_actor_n_finished_dev(const hsad_actor* actor);   /* device counter: sequences flushed by the last step */
hsad_seqwriter* hsad_actor_writer(hsad_actor* actor);
int hsad_actor_state(hsad_actor* actor, float** h, float** c);       /* the carried state entering the next step, fp32 [L, G*P, H] */
const int64_t* hsad_actor_last_actions(const hsad_actor* actor, const int64_t** greedy);   /* int64 [G*P] of the last step */
/* n-step priorities the last step pushed, float32 [*n] (per (game, player) row, VDN: per game); NULL when that step was still
 * filling the n-step window */
const float* hsad_actor_last_priority(const hsad_actor* actor, int32_t* n);

/* ---- The partnered actor: train next to fixed partners.  In every game some rows g * P + p belong to the learner and the rest to
 * rule-list bots (HSAD_RULE_*, above); the network runs on the learner's rows only, and only those rows reach the replay.
 *
 * hsad_actor_partners: every array is a HOST array; the actor copies what it needs to the device itself.
 *   rows      int32 [M]: the learner's rows g * P + p, strictly ascending, 1 <= M <= G * P.
 *   rules, n_rules, n_bot: the rule table exactly as hsad_env_policy_rule takes it (rules [n_bot][HSAD_RULE_MAX_RULES], n_rules
 *             [n_bot], 1 <= n_bot <= HSAD_RULE_MAX_BOTS); n_bot = 0 (rules and n_rules may then be NULL) only when M == G * P.
 *   seat_bot  int32 [G * P]: -1 on exactly the learner's rows, a bot index 0 .. n_bot - 1 on every other row.
 *   bot_seed  the seed of the bots' *_RANDOM rules (the `seed` of hsad_env_policy_rule).
 *
 * hsad_actor_create_partnered: an actor that behaves like an IQL actor of hsad_actor_create with E = M environments:
 *   - the LSTM state rings, the Q ring and the arena are sized by M; hsad_actor_state returns fp32 [L, M, H];
 *   - hsad_r2d2_act is called with N = M on compact rows in `rows` order (compact row e is row rows[e] of the env's outputs), so a
 *     row's index in the eps-greedy hash is its compact index e, not its row id;
 *   - the sequence writer has M envs; its fields are the learner rows' observation bits, legal bits, eps, own-hand bits, a and
 *     greedy_a (the transition layout of hsad_actor_io with m = 1: the replay is created as for an IQL actor);
 *   - reward and terminal of env e are those of game rows[e] / P; the carried state rows of env e are zeroed on that game's terminal;
 *   - both tail paths work on M envs: the one-launch tail hsad_seqwriter_step_tail, and the four entry points with the redo of
 *     Q_online(s_{t-n}, a) on M rows after a weight sync; hsad_actor_last_priority returns float32 [M];
 *   - every partner row gets the move of its bot as hsad_env_policy_rule(rules, n_rules, n_bot, seat_bot, bot_seed, key = NULL)
 *     defines it on the state the step starts from: the same hash streams 128 + 16 p + j, the game index as the key, the game's
 *     policy counter read once and advanced once per step in every game that has a bot (a game with no bot keeps its counter), the
 *     noop for a seat that is not on turn, greedy_a = a;
 *   - a learner row receives what hsad_seat_scatter would write: the agent's a / greedy_a (the noop in a game that is not live);
 *   - hsad_actor_num_act counts M per step; hsad_actor_last_actions returns the full int64 [G, P] arrays the env stepped with.
 * With rows = every row and n_bot = 0 the actor computes, bit for bit, what an actor of hsad_actor_create computes.
 * One step adds three launches to hsad_actor_step's: the row gather in front of act (bf16 observation row, float legal row, eps and
 * the three bit rows of the M rows into compact buffers), the action merge behind it (one thread per game), and the gather's second
 * pass behind the env step (reward / terminal per learner row).
 *
 * HSAD_ERR_INVALID with a message that names the offending entry, before anything is allocated or launched: cfg->vdn != 0; more
 * than 5 players; M outside 1 .. G * P; a rows entry out of range, or not above the entry before it (unsorted or duplicated);
 * n_bot outside 0 .. HSAD_RULE_MAX_BOTS, or 0 with partner rows; an n_rules entry outside 1 .. HSAD_RULE_MAX_RULES; an unknown rule
 * code; k out of range; a learner row whose seat_bot entry is not -1; a partner row whose entry is outside 0 .. n_bot - 1; and what
 * hsad_actor_create refuses (a skip_connect net, a missing buffer).  The check is csrc/hsad_partner.h. */
typedef struct hsad_actor_partners {
  const int32_t* rows;
  int32_t M;
  const hsad_rule* rules;
  const int32_t* n_rules;
  int32_t n_bot;
  const int32_t* seat_bot;
  uint64_t bot_seed;
} hsad_actor_partners;
int hsad_actor_create_partnered(hsad_env* env, hsad_r2d2_net* online, hsad_r2d2_net* target, hsad_replay* replay,
                                const hsad_actor_config* cfg, const hsad_actor_io* io, const hsad_actor_partners* partners,
                                hsad_actor** out);

/* ---- Frozen networks as partners.  A partner row belongs either to a rule-list bot, as above, or to one of up to
 * HSAD_PARTNER_MAX_NETS frozen networks.  A network partner acts greedily, carries its own LSTM state over the rows it owns and never
 * reaches the replay; the learner's side is what hsad_actor_create_partnered describes.
 *
 * hsad_actor_net_partners:
 *   nets      [n_net] handles, caller-owned and alive as long as the actor, on the actor's device; inference nets are enough.  Any
 *             architecture hsad_r2d2_act runs (num_fc_layer 1..2, num_lstm_layer 1..3, skip_connect, its own hid_dim): a partner needs no
 *             cached Q-values, so the skip_connect refusal of hsad_actor_create holds for the learner only.  in_dim and num_action
 *             must be the env's (and so the padded row length the learner's).  No handle twice, none equal to online or target: two act
 *             calls never share a workspace (the caller makes a copy).
 *   n_net     1 .. HSAD_PARTNER_MAX_NETS.
 *   seat_net  HOST int32 [G * P]: k on the rows of net k, -1 on every other row.
 * Every row has exactly one owner: the learner (rows), a bot (seat_bot[r] >= 0, seat_net[r] == -1) or a net (seat_net[r] >= 0,
 * seat_bot[r] == -1).  Net k owns n_k >= 1 rows; the compact index of a row of net k is its rank among them in ascending row order.
 * n_bot == 0 is allowed whenever no row is a bot's.
 *
 * Per step, on the caller's stream and in this order: the learner's hsad_r2d2_act, then for k = 0 .. n_net - 1
 *   hsad_r2d2_act(net_k, NULL, n_k, NULL, obs16_k, legal_k, eps = NULL, ..., q_online_a = NULL, q_target_greedy = NULL)
 * (greedy: a == greedy_a; no target pass; seed = cfg->seed, counter = the step number).  Act calls are never put on different
 * streams.  The state of net k ping-pongs between two slots and is zeroed on the terminal of the row's game (hsad_zero_state_rows,
 * per-row flags); the bf16 state copy is carried iff n_k >= 1024.  A partner row of a game that is not live receives the noop, as
 * hsad_seat_scatter writes it.  The weights are read through the handle on every step: weights written and refreshed on the same
 * stream between two steps take effect at the next step.
 * The compact rows of the learner and of all nets live in one index space (e < M: the learner; [off_k, off_k + n_k): net k): one
 * gather launch of M + sum n_k workgroups in front of the acts (a net row gets its bf16 observation row and its legal row only) and
 * one second pass behind the env step (terminal of every compact row, reward of the learner's) replace the two gather launches of
 * hsad_actor_create_partnered; the merge is the same kernel.  With net_partners == NULL the call IS hsad_actor_create_partnered.
 *
 * Refused on top of hsad_actor_create_partnered's list, before anything is allocated or launched: n_net out of range; a net whose
 * in_dim or num_action is not the env's; a seat_net entry on a learner row, on a bot's row, or outside -1 .. n_net - 1; a partner row
 * owned by nobody; a net that owns no row (csrc/hsad_partner.h, partner_layout_verdict_nets); a NULL, repeated, online or target handle.
 *
 * hsad_actor_partner_state: the carried state of net k entering the next step, fp32 [L_k, n_k, H_k]; *n_rows = n_k. */
enum { HSAD_PARTNER_MAX_NETS = 8 };
typedef struct hsad_actor_net_partners {
  hsad_r2d2_net* const* nets;
  int32_t n_net;
  const int32_t* seat_net;
} hsad_actor_net_partners;
int hsad_actor_create_partnered_nets(hsad_env* env, hsad_r2d2_net* online, hsad_r2d2_net* target, hsad_replay* replay,
                                     const hsad_actor_config* cfg, const hsad_actor_io* io, const hsad_actor_partners* partners,
                                     const hsad_actor_net_partners* net_partners, hsad_actor** out);
int hsad_actor_partner_state(hsad_actor* actor, int k, float** h, float** c, int32_t* n_rows);
/* Net partner k plays its softmax policy at temperature tau from the next step on: its per-step call becomes
 *   hsad_r2d2_act_soft(net_k, n_k, NULL, obs16_k, legal_k, eps = NULL, temp_k, row_key = NULL, 0, ..., seed = cfg->seed, counter = the
 *   step number, ..., q_online_a = NULL)
 * with temp_k [n_k] = tau on every row (a vector in the partner arena; the setter waits for the device and fills it with a blocking copy).  tau = 0 restores the hsad_r2d2_act
 * call above: a partner whose temperature was never set keeps today's launches.  tau < 0 or not finite is refused.  The learner's
 * rows are not touched, and nothing of a partner reaches the replay, as before. */
int hsad_actor_set_partner_temperature(hsad_actor* actor, int k, float tau);

/* ---- seat kernels of a tournament batch (eval.play_seatings): one env object holds every seating of a model pool over the same
 * deals (hsad_env_reseed with period = deals); a model acts once per step on the rows it owns, listed as flat row ids g * P + p.
 * All three are HBM-bound, one pass, launch-only. ---- */
/* One model's act operands in one launch: for i < n, row r = rows[i] of the env outputs ->
 *   obs_out row i:   obs_kind 0: bf16 [n, Kp] copied from priv_s_bf16 [*, Kp] (hsad_env_bind_packed rows, 16-byte vectors)
 *                    obs_kind 1: bf16 [n, Kp] cast and zero-padded from priv_s fp32 [*, F] (= hsad_cast_pad_bf16 of the rows)
 *                    obs_kind 2: fp32 [n, F] copied from priv_s (agents that take the float32 observation)
 *   legal_out row i: fp32 [n, A] copied from legal_move [*, A].
 * rows device int32 [n], each in [0, num_rows) (checked on the device; an id outside leaves its output row untouched). */
int hsad_seat_gather(const int32_t* rows, int n, int num_rows, int obs_kind, const void* obs_src, int F, int Kp, const float* legal_move,
                     int A, void* obs_out, float* legal_out, void* stream);
/* A model's chosen actions back into a / greedy_a int64 [G, P] at its rows; rows of finished (or not started) games receive the
 * noop uid A - 1, which hsad_env_step ignores.  a_src / greedy_src int64 [n]. */
int hsad_seat_scatter(const hsad_env* env, const int32_t* rows, int n, const int64_t* a_src, const int64_t* greedy_src, int64_t* a,
                      int64_t* greedy_a, void* stream);
/* Per seating s (games [s * games_per_seating, (s + 1) * games_per_seating); G must be a multiple) from the latched last scores of
 * the finished games: stats int64 [S, 4] = sum score, sum score^2, perfect games (score == colors * ranks), finished games; and
 * *unfinished int32 = games of the whole env not finished yet -- the one word a host loop reads.  Integer sums: exact, order-free. */
int hsad_seating_stats(const hsad_env* env, int games_per_seating, int64_t* stats, int32_t* unfinished, void* stream);
/* Behaviour counters: what KIND of moves each seat of each seating makes.  A move classifier (csrc/hsad_behaviour.h: bh_classify)
 * looks at the position BEFORE the move and at the uid the seat on turn is about to play, and gives the increments of the
 * HSAD_BH_NSTAT counters below; the position is never modified and nothing is remembered from move to move.  This text is the
 * specification (csrc/hsad_behaviour.h follows it, tests/behaviour_ref.py restates it).  It uses the definitions of the rule-bot
 * section above for the mover p: pool, compat_i, n_i, play_i, dead_i, playable(t), dead(t), full[t], discards[t].
 *    #  name                  +1 (HINT_CARDS, INFO_SUM: +n) when the move is ...
 *    0  MOVES                 any play, discard or hint
 *    1  PLAY_OK               a play of slot i whose card is playable
 *    2  PLAY_FAIL             a play whose card is not playable
 *    3  PLAY_CERTAIN          a play of slot i with play_i == n_i (the mover's own knowledge: exactly the test of rule 1)
 *    4  DISCARD               a discard
 *    5  DISCARD_CERTAIN_DEAD  a discard of slot i with dead_i == n_i (the test of rule 8)
 *    6  HINT_COLOUR           a colour hint
 *    7  HINT_RANK             a rank hint
 *    8  HINT_CARDS            +n, the number of cards of the target hand the hint touches
 *    9  HINT_PLAYABLE         a hint that touches at least one card that is playable now
 *   10  LAST_COPY_LOST        a discard or failed play of a card of type t with !dead(t) and discards[t] == full[t] - 1 before the move
 *   11  INFO_SUM              +the information tokens available before the move (every counted move)
 *   12  LAST_LIFE             a failed play with life == 1 before it
 * The uid is decoded by the layout above: discard slot i = i, play slot i = H + i, colour hint = 2H + (o-1) C + colour, rank hint =
 * 2H + (P-1) C + (o-1) R + rank, noop = A - 1.  With shuffle_color a colour hint names its colour through the ACTOR's permutation,
 * as its legal_move row does; the classifier maps it back to the cards' colour.  The noop, a uid outside [0, A), a play or discard
 * of an empty slot, and a hint that touches no card count NOTHING, not even MOVES (the env refuses and logs those; whether the
 * tokens allow a hint or a discard is the env's business too and is not looked at here).
 *
 * hsad_seating_behaviour: a device int64 [G, P], the rows about to go into hsad_env_step; counts device int64 [S, P, HSAD_BH_NSTAT],
 * S = G / games_per_seating.  For every live game g (started and not terminated) with seat p on turn:
 *   counts[g / games_per_seating][p] += bh_classify(planes of g, p, a[g, p]);
 * games that are not live add nothing.  It ACCUMULATES (as hsad_search_job_stats does): the caller zeroes counts.  Integer atomics
 * only: exact, order-free.  Reads the state planes and `a`, writes nothing but counts.  HSAD_ERR_INVALID before any launch: a null
 * argument, games_per_seating < 1 or not dividing G, more than 5 players.  Launch-only. */
enum {
  HSAD_BH_MOVES = 0,
  HSAD_BH_PLAY_OK = 1,
  HSAD_BH_PLAY_FAIL = 2,
  HSAD_BH_PLAY_CERTAIN = 3,
  HSAD_BH_DISCARD = 4,
  HSAD_BH_DISCARD_CERTAIN_DEAD = 5,
  HSAD_BH_HINT_COLOUR = 6,
  HSAD_BH_HINT_RANK = 7,
  HSAD_BH_HINT_CARDS = 8,
  HSAD_BH_HINT_PLAYABLE = 9,
  HSAD_BH_LAST_COPY_LOST = 10,
  HSAD_BH_INFO_SUM = 11,
  HSAD_BH_LAST_LIFE = 12,
  HSAD_BH_NSTAT = 13
};
int hsad_seating_behaviour(const hsad_env* env, int games_per_seating, const int64_t* a, int64_t* counts, void* stream);

/* ---- glue kernels of blueprint-policy search (search.PolicySearch): a search env of G slots plays (root game, candidate action,
 * sampled world) jobs with the R2D2 agent acting for every seat; hsad_env_fork + hsad_env_determinize place the worlds, these three
 * keep the rest of a chunk on the device.  All three are HBM-bound, one pass, launch-only. ---- */
/* The agent's carried state into the forks.  State tensors are fp32 [L, G * P, H], row (l, g * P + p).  For every layer l,
 * destination game j < G_dst and seat p < P: row (l, j * P + p) of h_dst / c_dst = row (l, src_index[j] * P + p) of h_src / c_src.
 * h16_dst (NULL = not wanted) bf16 [L, G_dst * P, H] receives the bf16 rounding (nearest even, as hsad_cast_pad_bf16) of the copied
 * h rows: the operand the fused cell reads for 1,024 rows or more (hid["h0_16"]).  src_index device int32 [G_dst]: -1 leaves the
 * rows of game j untouched, and so does any other value outside [0, G_src) (checked on the device, nothing is read out of bounds;
 * hsad_env_fork logs code 4 for the same list).  The source is only read; source and destination must not overlap.
 * HSAD_ERR_INVALID: H % 4 != 0, a size < 1, a null or not 16-byte aligned tensor. */
int hsad_search_fork_state(const int32_t* src_index, int G_dst, int G_src, int P, int L, int H, const float* h_src, const float* c_src,
                           float* h_dst, float* c_dst, void* h16_dst, void* stream);
/* The learned belief's features at search time (belief.BeliefSampler): the searcher's rows of the top LSTM layer's new h after the
 * root act, as the bf16 operand of the head's GEMM.  h_top fp32 [G * P, H] (row g * P + p), player device int32 [G], out_bf16 bf16
 * [G, ldo]: out[g, 0 .. H - 1] = bf16(h_top[g * P + player[g], :]), rounded to nearest even as hsad_cast_pad_bf16 does; an all-zero
 * row where player[g] is outside [0, P).  Columns H .. ldo - 1 are not written.  h_top is only read.  Rows move as 16-byte vectors:
 * HSAD_ERR_INVALID when H is no positive multiple of 8, ldo < H or ldo % 8 != 0, G or P < 1, a null or not 16-byte aligned tensor.
 * One pass, launch-only. */
int hsad_search_belief_rows(const float* h_top, const int32_t* player, int G, int P, int H, void* out_bf16, int ldo, void* stream);
/* What act returned for all G * P rows of `env` (a_src / greedy_src int64 [G * P]) -> what hsad_env_step takes (a / greedy_a int64
 * [G, P]; may be the same memory as the sources).  Every seat of a game that is finished or not started receives the noop uid A - 1
 * in both outputs.  In a live game g with override[g] >= 0 (device int64 [G]) and player[g] (device int32 [G]) in [0, P):
 * a[g, player[g]] = override[g]; greedy_a keeps greedy_src -- the agent's greedy action, what SAD shows the partner when the searcher
 * deviates.  A player outside [0, P) means no override for that game; override == NULL means masking only (player may be NULL too). */
int hsad_search_actions(const hsad_env* env, const int64_t* a_src, const int64_t* greedy_src, const int32_t* player,
                        const int64_t* override_a, int64_t* a, int64_t* greedy_a, void* stream);
/* Scores of the finished slots, reduced per job.  job device int32 [G]: the (root game, action) pair slot g works for; -1, or any
 * value outside [0, n_job), skips the slot.  For every finished game (started and terminated) with a valid job: stats int64
 * [n_job, 3] += (score, score^2, 1), where score is the score latched when the game ended -- HSAD_Q_SCORE of the final position
 * (0 after the last life with bomb = 1).  It ACCUMULATES: the caller zeroes stats once per search and calls this once per chunk.
 * Integer atomics: exact, order-free.  The "games still running" word of the host loop is hsad_seating_stats(env, G, ...)'s. */
int hsad_search_job_stats(const hsad_env* env, const int32_t* job, int n_job, int64_t* stats, void* stream);

/* ---- depth-limited search (PolicySearch(depth = D)): the worlds are played D + 1 moves and then valued as score so far + the
 * blueprint's own Q, in fixed point so that the reduction stays integer. ---- */
#define HSAD_SEARCH_VALUE_SCALE 256 /* a slot's value is an integer number of 1/256 points */
enum { HSAD_SEARCH_HORIZON_MOVER = 0, HSAD_SEARCH_HORIZON_TEAM = 1 };
/* hsad_search_job_stats for a search that stops at a horizon.  job as there; q_rows device fp32 [G * P]: Q_online(s, a) of every
 * row of `env` at the position it now holds (act(with_q) run on it, the env not stepped since).  Per slot g with a valid job
 * (the row function is csrc/hsad_search_horizon.h, S = HSAD_SEARCH_VALUE_SCALE):
 *   finished game (started and terminated): v = score * S with the score hsad_search_job_stats sums; the slot is not "cut".
 *   live game (started, not terminated): score = the sum of the fireworks (HSAD_Q_SCORE of a live board);
 *     q = q_rows[g * P + num_step % P], the row of the seat on turn (mode HSAD_SEARCH_HORIZON_MOVER), or the fp32 sum
 *     q_rows[g * P + 0] + ... + q_rows[g * P + P - 1] added in that order (mode HSAD_SEARCH_HORIZON_TEAM: VDN's joint value);
 *     b = (int)rintf(fminf(fmaxf(q, -64), 64) * S), round-half-even; a q that is NaN or infinite gives b = 0 and adds 1 to
 *     nonfinite[0]; v = min(max(score * S + b, 0), perfect_score * S); the slot is "cut".
 *   any other game (never started): nothing.
 * stats int64 [n_job, 3] += (v, v^2, 1), cut int64 [n_job] += 1 for a cut slot, nonfinite int64 [1].  All three ACCUMULATE
 * (the caller zeroes them once per search); 64-bit integer atomics only: exact, order-free.  world_values (NULL = not wanted)
 * device uint16 [n_job, worlds] with world device int32 [G]: world_values[job[g] * worlds + world[g]] = v for every counted slot
 * whose world lies in [0, worlds) -- plain 16-bit stores, a (job, world) is played once; the caller fills the table with 0xFFFF
 * ("not played") once per search.  `env` and q_rows are only read.
 * HSAD_ERR_INVALID before any launch: n_job <= 0, a mode other than the two, a null job / q_rows / stats / cut / nonfinite,
 * world_values without world, worlds <= 0 with world_values.  Launch-only, one pass. */
int hsad_search_horizon_stats(const hsad_env* env, const int32_t* job, int n_job, const float* q_rows, int mode, int64_t* stats,
                              int64_t* cut, int64_t* nonfinite, const int32_t* world, int worlds, uint16_t* world_values, void* stream);

/* ---- round-wise search (PolicySearch.search(rounds = ...)): the per-world scores are kept, so that actions can be compared world
 * by world (common random numbers: every action of a game meets the same worlds) and hopeless ones dropped between rounds. ---- */
/* The finished slots' scores, one byte each.  pair / world device int32 [G]: the (root game, action) pair and the world slot g
 * played.  For every finished game (started and terminated) with pair[g] in [0, n_pair) and world[g] in [0, worlds):
 * scores[pair[g] * worlds + world[g]] = the score hsad_search_job_stats sums, 0..25.  scores device uint8 [n_pair, worlds]; the
 * caller fills it with 0xFF ("not evaluated") once per search.  Every other slot stores nothing.  Plain byte stores, no atomics: a
 * (pair, world) is played at most once, and two slots of one call that named the same entry would race.
 * HSAD_ERR_INVALID: n_pair < 1, worlds < 1, a null argument. */
int hsad_search_world_scores(const hsad_env* env, const int32_t* pair, const int32_t* world, int n_pair, int worlds, uint8_t* scores,
                             void* stream);
/* One round's decision on the score table of hsad_search_world_scores.  Searched game k (one workgroup each) owns the pairs
 * first_pair[k] .. first_pair[k + 1] - 1 (device int32 [n_game + 1], ascending); bp_pair[k] (device int32 [n_game]) is the pair of
 * the blueprint's own action.  0xFF entries are absent.  All arithmetic is integer and no atomics are used: the outputs are the same
 * bits run to run.
 *   raw_out int64 [n_pair, 2] = (sum s, n) over the present entries of the row.
 *   leader_out int32 [n_game] = among the pairs with alive != 0 and n > 0 the one with the largest raw mean, compared exactly
 *     (sum_p * n_q > sum_q * n_p), ties to the lowest pair index; bp_pair[k] when there is no such pair.
 *   paired_ref_out / paired_bp_out int64 [n_pair, 3] = (D, Q, n) = (sum d, sum d^2, count) over the worlds present in both the pair's
 *     row and the leader's / the blueprint pair's row, d = s - s_ref.
 *   alive device uint8 [n_pair], read and written in place: a pair that is alive, is neither the leader nor bp_pair[k], is set to 0
 *     iff, with (D, Q, n) against the leader, n >= min_n, D < 0 and D^2 * n * z2_den > z2_num * (n * Q - D^2) -- its paired mean lies
 *     more than z standard errors (of the paired mean, population variance) below the leader's, z^2 = z2_num / z2_den.  Equality
 *     does not prune; z2_num = 0 prunes every negative D.
 * Bounds that keep every product in int64 (scores <= 25): worlds <= 4096, 1 <= z2_den <= 1024, 0 <= z2_num <= 16384, so that
 * D^2 * n * z2_den <= (25 * 2^12)^2 * 2^12 * 2^10 < 2^56.  HSAD_ERR_INVALID outside them, for min_n < 1, n_pair < 1, n_game < 1 and
 * null arguments.  Checked on the device: a game whose pair range is empty or leaves [0, n_pair) gets leader -1 and nothing else read
 * or written; a bp_pair[k] outside its game's range counts as "no blueprint pair": paired_bp_out is (0, 0, 0) for the game's pairs,
 * no pair is exempt on its account and the leader's fall-back is -1. */
int hsad_search_round(const uint8_t* scores, int n_pair, int worlds, const int32_t* first_pair, int n_game, const int32_t* bp_pair,
                      int z2_num, int z2_den, int min_n, uint8_t* alive, int32_t* leader_out, int64_t* raw_out, int64_t* paired_ref_out,
                      int64_t* paired_bp_out, void* stream);

/* ---- replay stage of blueprint-policy search (PolicySearch(replay = True)): every sampled world is played again from its first
 * move, so that each seat's LSTM state is the one that world's observations produce. ---- */
/* The deal script of every world slot.  world_env: a determinised fork of the root (G_w slots); src_index device int32 [G_w]: the
 * root game slot j was forked from; viewer device int32 [G_w]: the seat whose hand was resampled; root_deck_hist device uint8
 * [G_root, 52] and root_count device int32 [G_root]: the root's deck history and the number of cards it has dealt; log_a device
 * int64 [n_moves, G_root, P]: the action rows the root was stepped with, move after move.  Per slot j with s = src_index[j],
 * v = viewer[j]:
 *   slot list = deal indices v * H .. v * H + H - 1 (the initial deal gives seat p the indices p * H ..);  d = P * H;
 *   for t = 0 .. n_moves - 1: mover m = t mod P (movers rotate from seat 0), uid = log_a[t, s, m]; uid in [0, H) discards and
 *   uid in [H, 2H) plays hand slot i = uid mod H (the env's move-uid order); any other uid moves no card.  For a play or discard:
 *   if m == v, entry i leaves the list and the later entries shift down;  then, if d < root_count[s], a card was dealt to the
 *   mover: if m == v, d is appended to the list; d += 1.
 *   script_out[j] = root_deck_hist[s] (entries [0, root_count[s]), zero beyond) with entry list[k] replaced by card k of the hand
 *   world_env holds for seat v;  count_out[j] = root_count[s].
 * s = -1 or outside [0, G_root), v outside [0, P), root_count[s] < P * H (never started) or a log that does not lead to the length
 * of the hand world_env holds skip the slot: count_out[j] = 0 and an all-zero row, which hsad_env_rewind_scripted leaves alone
 * (the convention of hsad_env_fork and hsad_search_fork_state).  script_out device uint8 [G_w, 52], count_out device int32 [G_w]. */
int hsad_search_world_script(const hsad_env* world_env, const int32_t* src_index, const int32_t* viewer, const uint8_t* root_deck_hist,
                             const int32_t* root_count, int G_root, const int64_t* log_a, int n_moves, uint8_t* script_out,
                             int32_t* count_out, void* stream);
/* One teacher-forced replay step.  log_a_t / log_greedy_t device int64 [G_root, P]: the rows of move t of the root's log;
 * greedy_src device int64 [G * P]: the greedy actions act has just returned for env's rows.  For every slot g of env (G slots) with
 * s = src_index[g] in [0, G_root) whose game is live: a[g] / greedy_a[g] (device int64 [G, P]) = row s of log_a_t / log_greedy_t, and
 * mismatch[g] (device int32 [G]) += 1 when the mover -- seat (env's step count of game g) mod P -- is not viewer[g] and
 * greedy_src[g * P + mover] != log_greedy_t[s, mover]: in this world the blueprint would have shown another greedy action than the
 * one that was observed.  The logged greedy action is hypothetical and may be illegal in this world (a hint that touches no card of
 * the hand the world gave the viewer; the logged move itself is legal in every world the sampler gives): greedy_a[g, mover] is then
 * the logged move, so that the step accepts it, and the mismatch is counted all the same (act returns legal greedy actions only).
 * Finished, never-started and skipped (s outside [0, G_root)) slots get the noop uid A - 1 in both outputs.
 * mismatch ACCUMULATES: the caller zeroes it before move 0.  With sad = 1 the caller follows the step with hsad_env_observe_sad and
 * the logged section of this move, so that the rows show the greedy action as it was seen. */
int hsad_search_replay_actions(const hsad_env* env, const int32_t* src_index, const int32_t* viewer, const int64_t* log_a_t,
                               const int64_t* log_greedy_t, int G_root, const int64_t* greedy_src, int64_t* a, int64_t* greedy_a,
                               int32_t* mismatch, void* stream);

/* ---- Game records: which game, and show it to me.  A tournament's counters say how often; a record is one game written down --
 * its rules, its deal, every move with its greedy alternative and a flag byte from the move classifier, and how it ended -- so that
 * it can be filtered on the device, read on the host and replayed to any move in one launch.  The reference has no such call;
 * nothing below changes what reset / step / rollout or the existing playouts compute.  csrc/hsad_game_record.h holds the layout.
 *
 * Capacity.  With D = max deck size - P * H: exactly D plays + discards are made while the deck holds a card (each deals one), at
 * most max_information_tokens + D + colors hints (a hint spends a token; tokens come from the initial stock, from discards and
 * from completed stacks), and the last round adds P turns: a game has at most
 *     L = 2 * D + max_information_tokens + colors + P      (95 for the standard 2-player game)
 * moves.  A log whose game is at move index >= L counts an overflow instead of writing.  L > 255 is refused (HSAD_ERR_INVALID: the
 * env counts steps in 8 bits).
 *
 * The record, hsad_game_record_bytes(env) = 68 + 3 L bytes, every field one byte:
 *    0 version (HSAD_GR_VERSION)   1 P   2 H   3 colors   4 ranks   5 max_information_tokens   6 max_life_tokens   7 bomb
 *    8 n_moves   9 n_dealt   10 score (the latched last score of a finished game, the fireworks' sum of a running one, 0 after a
 *    bomb)   11 lives   12 information tokens   13 how it ended (HSAD_GR_END_*)   14 L   15 0
 *    16..67 the deck: card types (colour * 5 + rank) in deal order, 0 past n_dealt -- the deck-history row, the layout of a script
 *    68.. move[L], greedy[L], flags[L], 0 past n_moves
 * move / greedy: the uid (layout: hsad_seating_behaviour above) the mover played / would have played greedily, with a colour
 * hint's colour as the cards' TRUE colour: with shuffle_color the actor's permutation is undone, as bh_classify undoes it.
 * flags: HSAD_GR_* bits, read off the increments bh_classify gives for the move on the position before it:
 *    COUNTED            MOVES != 0 (every other bit is 0 without it)
 *    PLAY_FAIL          PLAY_FAIL
 *    PLAY_UNCERTAIN     a play (PLAY_OK or PLAY_FAIL) without PLAY_CERTAIN
 *    LAST_COPY_LOST     LAST_COPY_LOST
 *    LAST_LIFE          LAST_LIFE
 *    HINT_NOT_PLAYABLE  a hint (HINT_COLOUR or HINT_RANK) without HINT_PLAYABLE
 *    DISCARD_UNCERTAIN  a DISCARD without DISCARD_CERTAIN_DEAD
 *    NO_INFO            INFO_SUM == 0: made with no information token available
 * Move k is made by seat k % P (seat 0 opens, every move passes the turn on). */
#define HSAD_GR_VERSION 1
enum {
  HSAD_GR_COUNTED = 1, HSAD_GR_PLAY_FAIL = 2, HSAD_GR_PLAY_UNCERTAIN = 4, HSAD_GR_LAST_COPY_LOST = 8, HSAD_GR_LAST_LIFE = 16,
  HSAD_GR_HINT_NOT_PLAYABLE = 32, HSAD_GR_DISCARD_UNCERTAIN = 64, HSAD_GR_NO_INFO = 128
};
/* how a game ended: no life left, the turns after the last card used up, every firework complete, max_len reached */
enum { HSAD_GR_END_UNFINISHED = 0, HSAD_GR_END_LIVES = 1, HSAD_GR_END_DECK = 2, HSAD_GR_END_PERFECT = 3, HSAD_GR_END_MAX_LEN = 4 };
/* negative status words of hsad_env_playout_logged */
enum { HSAD_GR_STATUS_SKIPPED = -1, HSAD_GR_STATUS_REFUSED = -2, HSAD_GR_STATUS_BAD_INDEX = -3 };

/* which finished games hsad_game_log_select keeps: score in [score_min, score_max], lives left <= max_lives, n_moves in
 * [moves_min, moves_max], end_mask == 0 or bit (1 << HSAD_GR_END_*) of it set, and flag_mask == 0 or some move k whose seat k % P
 * is in seat_mask (seat_mask == 0: every seat) carries a flag of flag_mask. */
typedef struct hsad_game_filter {
  int32_t score_min, score_max, max_lives, moves_min, moves_max, end_mask, seat_mask, flag_mask;
} hsad_game_filter;

typedef struct hsad_game_log hsad_game_log;

/* A log for `env`'s games: three time-major byte planes [L, Gpad] (an append and the gather touch consecutive bytes across a
 * wave), a move count per game and an overflow counter, all zero.  HSAD_ERR_STATE when the env does not track its deck history
 * (the record needs the deal) or is not bound; HSAD_ERR_INVALID when L > 255.  The log keeps `env`'s sizes, not the env. */
int hsad_game_log_create(const hsad_env* env, hsad_game_log** out);
void hsad_game_log_destroy(hsad_game_log* log);
int hsad_game_log_clear(hsad_game_log* log, void* stream);
int hsad_game_log_capacity(const hsad_game_log* log);                 /* L */
int64_t hsad_game_record_bytes(const hsad_env* env);                   /* 68 + 3 L; 0 for a null env */
/* overflows counted since creation / the last clear; synchronises the device */
int hsad_game_log_overflow_count(hsad_game_log* log, int32_t* count);
/* Called where hsad_seating_behaviour is called: a / greedy_a device int64 [G, P] hold every seat's action, the env is not yet
 * stepped.  One lane per game: for a live game (started, not terminated) with seat p on turn and 0 <= a[g, p] < A - 1 it writes
 * move, greedy and flags at index HSAD_Q_NUM_STEP of game g and sets the game's move count to that index + 1.  Finished and
 * never-started games, the noop and a uid outside [0, A) write nothing; a greedy uid outside [0, A - 1) is logged as the move.
 * greedy_a may be NULL (greedy = move).  Launch-only. */
int hsad_game_log_append(hsad_game_log* log, const hsad_env* env, const int64_t* a, const int64_t* greedy_a, void* stream);
/* Stable stream compaction: index_out (device int32 [G]) receives, ascending, the games that are finished and pass `filter`
 * (NULL: every finished game) and have take[g] != 0 (take device uint8 [G], or NULL); *n_out (device int32) their number.  Three
 * launches (count, scan, write), no atomics: the same bits run to run.  Entries of index_out past n_out are not written. */
int hsad_game_log_select(hsad_game_log* log, const hsad_env* env, const hsad_game_filter* filter, const uint8_t* take,
                         int32_t* index_out, int32_t* n_out, void* stream);
/* The records of games index[0 .. n) (device int32, each in [0, G); others give an all-zero record), contiguous in `out` (device
 * uint8 [n, hsad_game_record_bytes]).  The result fields come from the env's planes, the deck from its deck history, the moves
 * from the log: gather before the env is reset.  Only these bytes need to cross to the host. */
int hsad_game_log_gather(hsad_game_log* log, const hsad_env* env, const int32_t* index, int n, uint8_t* out, void* stream);
/* Replay: game j of a started env becomes record src_index[j] (device int32 [G]) played from its first deal up to move
 * min(stop[j], n_moves) (stop device int32 [G], or NULL: to the end), in one launch.  -1 leaves game j alone (status
 * HSAD_GR_STATUS_SKIPPED), any other index outside [0, n_rec) is logged as code 4 (HSAD_GR_STATUS_BAD_INDEX).  records: HOST
 * memory, n_rec records of hsad_game_record_bytes(env) each; a record of another version, other rules (P, H, colors, ranks, token
 * limits, bomb), another capacity, n_moves > L or n_dealt > 52 is refused with HSAD_ERR_INVALID before anything is launched.
 * The game is first rewound as hsad_env_rewind_scripted rewinds it, with the record's deck as its script, and that call's rules
 * hold: eps, colour permutations, generator and policy counter are kept, the env holds a deal script afterwards; a deck the rules
 * cannot deal is code 5 and a game that was never started is left alone (both HSAD_GR_STATUS_REFUSED).  Then one wave per 64
 * games plays the moves with the planes and the records' move planes staged in LDS, dealing from the script; no observation row
 * is written during the replay.  A logged colour hint is mapped forward through the mover's colour permutation.  Before each move
 * the mover's legal mask is consulted: an illegal logged move (or, with sad = 1, greedy move) stops that game at the position
 * before it and is logged as code 8.  status[j] (device int32 [G]) = the number of moves played, which for a stopped game is the
 * index of the refused move.  Afterwards the look-ahead, planes, `terminal` and legal masks are current as after a playout, and
 * the observe pass runs as after hsad_env_import_state: rows current, SAD section all-zero, reward 0.  Launch-only. */
int hsad_env_playout_logged(hsad_env* env, const uint8_t* records, int n_rec, const int32_t* src_index, const int32_t* stop,
                            int32_t* status, void* stream);

/* ---- one-sided intra-node transport (dist.py ReplayLink(transport = "ipc")): landing buffers exported by IPC handle and written by the
 * SENDER with a device-to-device copy -- SDMA over xGMI, no kernel resident on either GPU while a peer has not answered (a posted RCCL
 * receive is one, and the learner's whole-chip persistent launches cannot start next to it).  Completion is announced by the sender's
 * host through the rendezvous store.  Needs HSA_ENABLE_IPC_MODE_LEGACY=0 (dmabuf IPC). ---- */
int hsad_ipc_handle_bytes(void);
int hsad_ipc_alloc(int64_t bytes, void** dev_ptr, void* handle_out, int handle_bytes);   /* zero-filled device memory + its handle */
int hsad_ipc_free(void* dev_ptr);
int hsad_ipc_open(const void* handle, void** dev_ptr);                                    /* map a peer's allocation */
int hsad_ipc_close(void* dev_ptr);
int hsad_ipc_put(void* dst_mapped, const void* src, int64_t bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* HSAD_H_ */
