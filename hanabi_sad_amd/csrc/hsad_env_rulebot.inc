// hsad_env_rulebot.inc — rule-list bots (hsad_rulebot.h) as a policy of the env: one policy call on the planes in global memory, and
// whole playouts in one launch with the planes in LDS.  Textually part of hsad_env.hip (included at its end: the kernels below use
// its state planes, its game logic and the playout body of hsad_env_search.inc as they are).
//
// Nothing here is reached by reset / step / rollout: the two kernels are separate launches and EnvParams is what it was.  The
// playout kernel shares playout_body with env_playout_kernel (playout_random); the step and rollout kernels are compiled from
// unchanged code.  Plain loads and vector stores only; the one atomic is log_error's.

#include "hsad_rulebot.h"

namespace {

static_assert(kRbPlaneStride == kWave, "LdsPlanes (hsad_rulebot.h) indexes the planes as the kernels stage them: [npl][kWave]");

// ---- one policy call: one thread per game on the planes in global memory, the shape of policy_kernel ----------------------------------
__global__ __launch_bounds__(256) void policy_rule_kernel(EnvParams ep, RuleBots rb, const int32_t* __restrict__ seat_bot, uint64_t seed,
                                                          const int64_t* __restrict__ key, int64_t* __restrict__ a,
                                                          int64_t* __restrict__ ga) {
  __shared__ uint32_t s_rb[kRuleBotWords];
  stage_bots(rb, s_rb, threadIdx.x, blockDim.x);
  const int g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= ep.G) return;
  const int P = ep.P;
  bool any = false;
  for (int p = 0; p < P; ++p) any |= seat_bot[(size_t)g * P + p] != -1;
  if (!any) return;
  const uint32_t counter = ep.act_count[g];
  ep.act_count[g] = counter + 1u;
  const RbRules ru = rb_rules_of(ep);
  const GlobalPlanes w = {ep.planes, (size_t)ep.Gpad, g};
  const uint64_t k64 = key ? (uint64_t)key[g] : (uint64_t)g;
  for (int p = 0; p < P; ++p) {
    const int b = seat_bot[(size_t)g * P + p];
    if (b == -1) continue;
    if (b < 0 || b >= rb.n_bot) {
      log_error(ep, g, 7);
      continue;
    }
    const int uid = rb_act(w, ru, p, s_rb, b, seed, k64, (uint64_t)counter, nullptr);
    a[(size_t)g * P + p] = uid;
    if (ga) ga[(size_t)g * P + p] = uid;
  }
}

// ---- playout: bot -> step until the games end ------------------------------------------------------------------------------------------
// playout_body (hsad_env_search.inc) with the bot of the seat on turn as its policy.  The bot reads the planes where they are
// (LdsPlanes); its per-slot sums are 15 registers of the lane.
struct RuleBotPolicy {
  RbRules rr;             // the env's rules, with the kernel's compile-time players / hand size
  LdsPlanes w;            // the lane's game in the staged planes
  const uint32_t* s_rb;   // the staged RuleBots
  template <int TH, class Ru>
  __device__ __forceinline__ void act(const EnvParams& ep, const uint32_t* s_st, int lane, int g, int P, int H, const Ru& ru, uint64_t pkey,
                                      uint32_t counter) const {
    const int cur = board_cur(ST(PL_BOARD));
    // (a live game has a seat on turn; the bound keeps the LDS read in range whatever the planes hold)
    const int uid = (cur >= 0 && cur < P) ? rb_act(w, rr, cur, s_rb, (int)s_rb[RB_TABLE_WORDS + cur], ep.policy_seed, pkey, (uint64_t)counter, nullptr)
                                          : ep.A - 1;
    for (int p = 0; p < P; ++p) {
      const int64_t v = p == cur ? uid : ep.A - 1;
      ep.a_out[(size_t)g * P + p] = v;
      if (ep.g_out) ep.g_out[(size_t)g * P + p] = v;
    }
  }
};

template <int TP, int TH, bool V>
__global__ __launch_bounds__(kWave) void env_playout_rule_kernel(EnvParams ep, RuleBots rb, const int64_t* __restrict__ key) {
  extern __shared__ __attribute__((aligned(16))) uint32_t smem[];   // the planes playout_body stages
  __shared__ uint32_t s_rb[kRuleBotWords];
  stage_bots(rb, s_rb, threadIdx.x, kWave);
  RbRules rr = rb_rules_of(ep);
  rr.P = TP ? TP : ep.P;
  rr.H = TH ? TH : ep.H;
  playout_body<TP, TH, V>(ep, key, RuleBotPolicy{rr, LdsPlanes{smem, (int)threadIdx.x}, s_rb});
}

typedef void (*EnvPlayoutRuleFn)(EnvParams, RuleBots, const int64_t*);
EnvPlayoutRuleFn pick_playout_rule_kernel(const EnvParams& ep) {
  if (ep.variant) return env_playout_rule_kernel<0, 0, true>;
  if (ep.P == 2 && ep.H == 5) return env_playout_rule_kernel<2, 5, false>;
  return env_playout_rule_kernel<0, 0, false>;
}

// the caller's lists -> the launch's table; every refusal of the two entry points that concerns the lists
int make_bots(const char* who, const hsad_env* e, const hsad_rule* rules, const int32_t* n_rules, int n_bot, RuleBots* rb) {
  if (!rules || !n_rules) return set_error(HSAD_ERR_INVALID, "%s: null rule lists", who);
  if (e->ep.P > 5 || e->ep.H > 5) return set_error(HSAD_ERR_INVALID, "%s: more than 5 players or 5 cards a hand", who);
  if (n_bot < 1 || n_bot > HSAD_RULE_MAX_BOTS) return set_error(HSAD_ERR_INVALID, "%s: n_bot = %d, must be 1..%d", who, n_bot, HSAD_RULE_MAX_BOTS);
  memset(rb, 0, sizeof(*rb));
  rb->n_bot = n_bot;
  for (int b = 0; b < n_bot; ++b) {
    const hsad_rule* r = rules + (size_t)b * HSAD_RULE_MAX_RULES;
    switch (rb_rules_invalid(r, n_rules[b])) {
      case 1: return set_error(HSAD_ERR_INVALID, "%s: bot %d has %d rules, must be 1..%d", who, b, n_rules[b], HSAD_RULE_MAX_RULES);
      case 2: return set_error(HSAD_ERR_INVALID, "%s: bot %d names an unknown rule code", who, b);
      case 3: return set_error(HSAD_ERR_INVALID, "%s: bot %d: k must be 0..100 for the PROBABLE rules and 0 for every other", who, b);
      default: break;
    }
    for (int j = 0; j < n_rules[b]; ++j) rb->table[b * HSAD_RULE_MAX_RULES + j] = rb_pack(r[j].code, r[j].k);
    rb->table[HSAD_RULE_MAX_BOTS * HSAD_RULE_MAX_RULES + b] = (uint32_t)n_rules[b];
  }
  return HSAD_OK;
}

}  // namespace

extern "C" {

int hsad_env_policy_rule(hsad_env* e, const hsad_rule* rules, const int32_t* n_rules, int n_bot, const int32_t* seat_bot, uint64_t seed,
                         const int64_t* key, int64_t* a, int64_t* greedy_a, void* stream) {
  if (!e) return set_error(HSAD_ERR_INVALID, "null env");
  if (!e->bound) return set_error(HSAD_ERR_STATE, "hsad_env_bind_outputs must be called first");
  if (!a || !seat_bot) return set_error(HSAD_ERR_INVALID, "hsad_env_policy_rule: action tensor or seat_bot is null");
  RuleBots rb;
  const int rc = make_bots("hsad_env_policy_rule", e, rules, n_rules, n_bot, &rb);
  if (rc != HSAD_OK) return rc;
  hipLaunchKernelGGL(policy_rule_kernel, dim3((e->ep.G + 255) / 256), dim3(256), 0, (hipStream_t)stream, e->ep, rb, seat_bot, seed, key, a,
                     greedy_a);
  HIP_TRY(hipGetLastError());
  return HSAD_OK;
}

// shared with csrc/hsad_actor.hip (not part of the public header): what a rule bot outside this file needs of an env -- the state
// planes [npl][Gpad], the policy counters [Gpad] and the rules rb_act takes, as policy_rule_kernel sees them
int hsad_internal_env_rulebot_view(const hsad_env* e, const uint32_t** planes, uint32_t** act_count, int* G, int* Gpad, RbRules* ru) {
  if (!e) return set_error(HSAD_ERR_INVALID, "null env");
  if (!e->bound) return set_error(HSAD_ERR_STATE, "hsad_env_bind_outputs must be called first");
  *planes = e->ep.planes;
  *act_count = e->ep.act_count;
  *G = e->ep.G;
  *Gpad = e->ep.Gpad;
  *ru = rb_rules_of(e->ep);
  return HSAD_OK;
}

int hsad_env_playout_rule(hsad_env* e, int max_iter, const hsad_rule* rules, const int32_t* n_rules, int n_bot,
                          const int32_t* seat_bot_of_seat, uint64_t seed, const int64_t* key, int64_t* a, int64_t* greedy_a, void* stream) {
  if (!e) return set_error(HSAD_ERR_INVALID, "null env");
  if (!e->bound) return set_error(HSAD_ERR_STATE, "hsad_env_bind_outputs must be called first");
  if (!a || !seat_bot_of_seat) return set_error(HSAD_ERR_INVALID, "hsad_env_playout_rule: action tensor or seat_bot_of_seat is null");
  if (e->ep.sad && !greedy_a) return set_error(HSAD_ERR_INVALID, "sad=1 requires greedy_a");
  if (max_iter < 0) return set_error(HSAD_ERR_INVALID, "max_iter must be >= 0");
  RuleBots rb;
  const int rc = make_bots("hsad_env_playout_rule", e, rules, n_rules, n_bot, &rb);
  if (rc != HSAD_OK) return rc;
  for (int p = 0; p < e->ep.P; ++p) {
    if (seat_bot_of_seat[p] < 0 || seat_bot_of_seat[p] >= n_bot)
      return set_error(HSAD_ERR_INVALID, "hsad_env_playout_rule: seat %d plays bot %d, must be 0..%d", p, seat_bot_of_seat[p], n_bot - 1);
    rb.seat[p] = seat_bot_of_seat[p];
  }
  if (e->scripted)
    return set_error(HSAD_ERR_STATE, "hsad_env_playout_rule: the env holds a deal script (only hsad_env_step deals from it; hsad_env_reset clears it)");
  if (max_iter == 0) return HSAD_OK;
  EnvParams ep = e->ep;
  ep.policy_seed = seed;
  ep.n_iter = max_iter;
  ep.a_out = a;
  ep.g_out = greedy_a;
  ep.dbg = nullptr;
  hipLaunchKernelGGL(pick_playout_rule_kernel(ep), dim3(ep.Gpad / kWave), dim3(kWave), sizeof(uint32_t) * (size_t)ep.npl * kWave,
                     (hipStream_t)stream, ep, rb, key);
  HIP_TRY(hipGetLastError());
  return HSAD_OK;
}

}  // extern "C"
