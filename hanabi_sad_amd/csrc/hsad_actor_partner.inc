// hsad_actor_partner.inc — the partnered actor (include/hsad.h: hsad_actor_create_partnered): in every game some rows g * P + p belong
// to the learner and the rest to rule-list bots (hsad_rulebot.h).  The network runs on the learner's M rows only, and only those rows
// reach the sequence writer and the replay.  Textually part of hsad_actor.hip (included behind struct hsad_actor: it uses the actor's
// state rings, its side streams and its tail as they are).
//
// Nothing here is reached by an actor of hsad_actor_create: hsad_actor_step branches on `partner` once.  Two kernels are on the
// step's path, both plain loads and vector stores, no atomics, no LDS beyond the staged bot table:
//   partner_gather_kernel<0>  one launch in front of act: everything act and the sequence writer read of the learner's rows, compact
//   partner_gather_kernel<1>  the same kernel's second pass behind the env step: reward and terminal of each learner row's game
//   partner_merge_kernel      one thread per game, between act and the env step: the full a / greedy_a [G, P] -- the learner's rows
//                             from the compact act output, the partners' from their bots on the state planes (policy_rule_kernel's
//                             sibling: the same rb_act, hash streams, default key and counter rule)
// With frozen network partners (hsad_actor_create_partnered_nets) a partner row may belong to a net instead of a bot: the two gather
// launches become partner_gather_nets_kernel<0> / <1> over the learner's and every net's rows, and one greedy hsad_r2d2_act per net
// follows the learner's on the same stream.  An actor without nets launches what it launched before.
#include "hsad_partner.h"

// csrc/hsad_env_rulebot.inc
extern "C" int hsad_internal_env_rulebot_view(const hsad_env* e, const uint32_t** planes, uint32_t** act_count, int* G, int* Gpad, RbRules* ru);

namespace {

constexpr int kPartnerGatherThreads = 192;   // 896 bf16 + 14 bit words + 21 floats + 3 words of a row are 143 pieces: one pass

// the pieces of one row, in the order the threads of a workgroup take them: obs vectors, bit-row pieces, legal pieces, three words
struct PartnerGather {
  const int32_t* rows;             // [M] learner rows g * P + p
  int M, P;
  // sources: the env's outputs (hsad_actor_io)
  const uint4* obs16;              // [G*P][Fp] bf16 as 16-byte vectors
  const float* legal;              // [G*P][A]
  const float* eps;                // [G*P]
  const unsigned long long* priv_bits;    // [G*P][pw64]
  const unsigned long long* legal_bits;   // [G*P]
  const unsigned long long* own_bits;     // [G*P]
  const float* reward;             // [G]
  const uint8_t* terminal;         // [G]
  // destinations, compact [M]
  uint4* c_obs16;
  float* c_legal;
  float* c_eps;
  unsigned long long* c_priv_bits;
  unsigned long long* c_legal_bits;
  unsigned long long* c_own_bits;
  float* c_reward;
  uint8_t* c_terminal;
  int n_obs;                       // Fp / 8 vectors of a row
  int pw64, pb_vec, n_pb;          // bit row: pw64 words; as n_pb = pw64 / 2 vectors when the width is even, else as pw64 words
  int A, lg_vec, n_lg;             // legal row: as n_lg = A / 4 vectors when 4 | A, else as A floats
};

// PASS 0: one workgroup per learner row.  PASS 1: one thread per learner row.
template <int PASS>
__global__ __launch_bounds__(kPartnerGatherThreads) void partner_gather_kernel(PartnerGather g) {
  if (PASS == 1) {
    const int e = blockIdx.x * kPartnerGatherThreads + threadIdx.x;
    if (e >= g.M) return;
    const int game = g.rows[e] / g.P;
    g.c_reward[e] = g.reward[game];
    g.c_terminal[e] = g.terminal[game];
    return;
  }
  const int e = blockIdx.x;   // < M: the grid is M workgroups
  const size_t r = (size_t)g.rows[e];
  const int total = g.n_obs + g.n_pb + g.n_lg + 3;
  for (int k = threadIdx.x; k < total; k += kPartnerGatherThreads) {
    int j = k;
    if (j < g.n_obs) {
      g.c_obs16[(size_t)e * g.n_obs + j] = g.obs16[r * g.n_obs + j];
      continue;
    }
    j -= g.n_obs;
    if (j < g.n_pb) {
      if (g.pb_vec)
        reinterpret_cast<uint4*>(g.c_priv_bits)[(size_t)e * g.n_pb + j] = reinterpret_cast<const uint4*>(g.priv_bits)[r * g.n_pb + j];
      else
        g.c_priv_bits[(size_t)e * g.pw64 + j] = g.priv_bits[r * g.pw64 + j];
      continue;
    }
    j -= g.n_pb;
    if (j < g.n_lg) {
      if (g.lg_vec)
        reinterpret_cast<float4*>(g.c_legal)[(size_t)e * g.n_lg + j] = reinterpret_cast<const float4*>(g.legal)[r * g.n_lg + j];
      else
        g.c_legal[(size_t)e * g.A + j] = g.legal[r * g.A + j];
      continue;
    }
    j -= g.n_lg;
    if (j == 0) g.c_eps[e] = g.eps[r];
    else if (j == 1) g.c_legal_bits[e] = g.legal_bits[r];
    else g.c_own_bits[e] = g.own_bits[r];
  }
}

// seat [G * P]: the bot b >= 0 of a partner row, or -(e + 1) for the learner row whose compact index is e.  A learner row of a game
// that is not live gets the noop, as hsad_seat_scatter gives it; a partner row gets what hsad_env_policy_rule gives it.
__global__ __launch_bounds__(256) void partner_merge_kernel(const uint32_t* __restrict__ planes, uint32_t* __restrict__ act_count, int G, int Gpad,
                                                            RbRules ru, RuleBots rb, const int32_t* __restrict__ seat, uint64_t seed,
                                                            const int64_t* __restrict__ a_c, const int64_t* __restrict__ g_c,
                                                            int64_t* __restrict__ a, int64_t* __restrict__ ga) {
  __shared__ uint32_t s_rb[kRuleBotWords];
  stage_bots(rb, s_rb, threadIdx.x, blockDim.x);   // (the seat words of rb are zero here and never read: seats are per row, `seat`)
  const int g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= G) return;
  const int P = ru.P;
  int32_t st[5];   // P <= 5 (refused otherwise)
  bool any = false;
#pragma unroll
  for (int p = 0; p < 5; ++p) {
    st[p] = p < P ? seat[(size_t)g * P + p] : -1;
    any |= p < P && st[p] >= 0;
  }
  const GlobalPlanes w = {planes, (size_t)Gpad, g};
  const bool live = misc_live(w(PL_MISC));
  uint32_t counter = 0u;
  if (any) {   // the policy counter: read once, advanced once per call in every game that has a bot
    counter = act_count[g];
    act_count[g] = counter + 1u;
  }
#pragma unroll
  for (int p = 0; p < 5; ++p) {
    if (p >= P) break;
    const size_t r = (size_t)g * P + p;
    if (st[p] >= 0) {
      const int uid = rb_act(w, ru, p, s_rb, st[p], seed, (uint64_t)g, (uint64_t)counter, nullptr);
      a[r] = uid;
      ga[r] = uid;
    } else {
      const int e = -st[p] - 1;
      a[r] = live ? a_c[e] : (int64_t)(ru.A - 1);
      ga[r] = live ? g_c[e] : (int64_t)(ru.A - 1);
    }
  }
}

// The gather of an actor with frozen network partners (hsad_actor_create_partnered_nets).  The compact rows of the learner and of
// every net share one index space: e < g.M is the learner's row e, [off_k, off_k + n_k) are the rows of net k; g.rows, c_obs16,
// c_legal and c_terminal hold n_all = M + sum n_k entries, every other compact buffer M.  A sibling of partner_gather_kernel, which an
// actor without nets keeps launching as it is.
//   PASS 0: one workgroup per compact row.  A learner row gets its 143 pieces; a net row only what hsad_r2d2_act reads, the bf16
//           observation row and the legal row (no bit rows, eps or own hand: it never reaches the writer).
//   PASS 1: one thread per compact row: the terminal flag of the row's game, and the reward for the learner's rows.
struct PartnerGatherNets {
  PartnerGather g;
  int n_all;
};

template <int PASS>
__global__ __launch_bounds__(kPartnerGatherThreads) void partner_gather_nets_kernel(PartnerGatherNets q) {
  const PartnerGather& g = q.g;
  if (PASS == 1) {
    const int e = blockIdx.x * kPartnerGatherThreads + threadIdx.x;
    if (e >= q.n_all) return;
    const int game = g.rows[e] / g.P;
    g.c_terminal[e] = g.terminal[game];
    if (e < g.M) g.c_reward[e] = g.reward[game];
    return;
  }
  const int e = blockIdx.x;   // < n_all: the grid is n_all workgroups
  const size_t r = (size_t)g.rows[e];
  const bool learner = e < g.M;   // (uniform over the workgroup)
  const int n_pb = learner ? g.n_pb : 0;
  const int total = g.n_obs + n_pb + g.n_lg + (learner ? 3 : 0);
  for (int k = threadIdx.x; k < total; k += kPartnerGatherThreads) {
    int j = k;
    if (j < g.n_obs) {
      g.c_obs16[(size_t)e * g.n_obs + j] = g.obs16[r * g.n_obs + j];
      continue;
    }
    j -= g.n_obs;
    if (j < n_pb) {
      if (g.pb_vec)
        reinterpret_cast<uint4*>(g.c_priv_bits)[(size_t)e * g.n_pb + j] = reinterpret_cast<const uint4*>(g.priv_bits)[r * g.n_pb + j];
      else
        g.c_priv_bits[(size_t)e * g.pw64 + j] = g.priv_bits[r * g.pw64 + j];
      continue;
    }
    j -= n_pb;
    if (j < g.n_lg) {
      if (g.lg_vec)
        reinterpret_cast<float4*>(g.c_legal)[(size_t)e * g.n_lg + j] = reinterpret_cast<const float4*>(g.legal)[r * g.n_lg + j];
      else
        g.c_legal[(size_t)e * g.A + j] = g.legal[r * g.A + j];
      continue;
    }
    j -= g.n_lg;   // (learner rows only)
    if (j == 0) g.c_eps[e] = g.eps[r];
    else if (j == 1) g.c_legal_bits[e] = g.legal_bits[r];
    else g.c_own_bits[e] = g.own_bits[r];
  }
}

}  // namespace

// a frozen network partner: its rows' slice of the compact index space and its carried state (two slots: act never writes the state
// it reads; nothing of a partner is ever redone, so no ring)
struct PartnerNet {
  hsad_r2d2_net* net = nullptr;
  int n = 0, off = 0, L = 0, H = 0;
  bool fused = false;              // n >= 1024: the bf16 copy of the state is carried (the learner's fused_state rule per net)
  float *h[2] = {nullptr, nullptr}, *c[2] = {nullptr, nullptr};
  void* h16[2] = {nullptr, nullptr};
  float* temp = nullptr;           // [n], every entry tau (hsad_actor_set_partner_temperature); read by the act call only while tau > 0
  float tau = 0.f;
};

// what a partnered actor holds on top of hsad_actor
struct PartnerSeats {
  char* arena = nullptr;
  PartnerGather g;                 // both passes' argument
  RuleBots bots;                   // the packed rule table; the seats are per row (`seat` below), not per launch
  RbRules ru;
  const uint32_t* planes = nullptr;
  uint32_t* act_count = nullptr;
  int Gpad = 0;
  int32_t* seat = nullptr;         // [G * P], see partner_merge_kernel
  int64_t *a_c = nullptr, *g_c = nullptr;   // compact act output [M] (with network partners [n_all]: every act call's slice)
  uint64_t bot_seed = 0;
  // hsad_actor_create_partnered_nets
  int n_net = 0, n_all = 0;        // n_all = M + sum n_k compact rows
  int net_cur = 0;                 // the state slot that enters the nets' next act
  uint64_t net_counter = 0;
  PartnerNet nets[HSAD_PARTNER_MAX_NETS];
};

namespace {

void partner_free(PartnerSeats* pt) {
  if (!pt) return;
  if (pt->arena) (void)hipFree(pt->arena);
  delete pt;
}

// hsad_actor_step of a partnered actor: hsad_actor_step's iteration with the gather in front of act, the merge behind it, and the
// tail on the gathered reward / terminal
int partner_step(hsad_actor* ac, void* stream) {
  PartnerSeats* pt = ac->partner;
  hipStream_t s = (hipStream_t)stream;
  const int M = ac->N;
  const int cur = ac->cur, nxt = (cur + 1) % ac->nslot;
  if (ac->reset_pending) ac->reset_pending = false;
  else CK(hsad_env_reset(ac->env, stream));
  const PartnerGatherNets gn = {pt->g, pt->n_all};
  if (pt->n_net) hipLaunchKernelGGL(partner_gather_nets_kernel<0>, dim3(pt->n_all), dim3(kPartnerGatherThreads), 0, s, gn);
  else hipLaunchKernelGGL(partner_gather_kernel<0>, dim3(M), dim3(kPartnerGatherThreads), 0, s, pt->g);
  HIP_TRY(hipGetLastError());
  const uint64_t v_on = hsad_r2d2_net_version(ac->online);
  CK(hsad_r2d2_act(ac->online, ac->target, M, nullptr, pt->g.c_obs16, pt->g.c_legal, pt->g.c_eps, ac->h[cur], ac->c[cur],
                   ac->fused_state ? ac->h16[cur] : nullptr, ac->seed, ac->counter++, pt->a_c, pt->g_c, ac->h[nxt], ac->c[nxt],
                   ac->fused_state ? ac->h16[nxt] : nullptr, ac->qring[cur], ac->tq, stream));
  ac->qversion[cur] = v_on;
  // the frozen networks, one after the other on the same stream (a net owns its workspace, and the recurrence launches exchange
  // through inter-workgroup counters: two act calls never run side by side): greedy, no target pass, no cached Q-values
  const int ncur = pt->net_cur, nnxt = ncur ^ 1;
  for (int k = 0; k < pt->n_net; ++k) {
    const PartnerNet& pn = pt->nets[k];
    if (pn.tau > 0.f) {   // the partner plays its softmax policy: the same net pass, the sampling tail
      CK(hsad_r2d2_act_soft(pn.net, pn.n, nullptr, pt->g.c_obs16 + (size_t)pn.off * pt->g.n_obs, pt->g.c_legal + (size_t)pn.off * pt->g.A, nullptr,
                            pn.temp, nullptr, 0, pn.h[ncur], pn.c[ncur], pn.fused ? pn.h16[ncur] : nullptr, ac->seed, pt->net_counter,
                            pt->a_c + pn.off, pt->g_c + pn.off, pn.h[nnxt], pn.c[nnxt], pn.fused ? pn.h16[nnxt] : nullptr, nullptr, stream));
      continue;
    }
    CK(hsad_r2d2_act(pn.net, nullptr, pn.n, nullptr, pt->g.c_obs16 + (size_t)pn.off * pt->g.n_obs, pt->g.c_legal + (size_t)pn.off * pt->g.A, nullptr,
                     pn.h[ncur], pn.c[ncur], pn.fused ? pn.h16[ncur] : nullptr, ac->seed, pt->net_counter, pt->a_c + pn.off, pt->g_c + pn.off,
                     pn.h[nnxt], pn.c[nnxt], pn.fused ? pn.h16[nnxt] : nullptr, nullptr, nullptr, stream));
  }
  pt->net_counter += 1;
  hipLaunchKernelGGL(partner_merge_kernel, dim3((ac->G + 255) / 256), dim3(256), 0, s, pt->planes, pt->act_count, ac->G, pt->Gpad, pt->ru, pt->bots,
                     pt->seat, pt->bot_seed, pt->a_c, pt->g_c, ac->a, ac->greedy);
  HIP_TRY(hipGetLastError());
  const void* fields[6] = {pt->g.c_priv_bits, pt->g.c_legal_bits, pt->g.c_eps, pt->g.c_own_bits, pt->a_c, pt->g_c};
  CK(hsad_seqwriter_push_obs_action(ac->writer, fields, stream));
  CK(hsad_env_step(ac->env, ac->a, ac->greedy, stream));
  HIP_TRY(hipEventRecord(ac->ev_main, s));
  HIP_TRY(hipStreamWaitEvent(ac->side_reset, ac->ev_main, 0));
  CK(hsad_env_reset(ac->env, (void*)ac->side_reset));
  HIP_TRY(hipEventRecord(ac->ev_reset, ac->side_reset));
  ac->reset_pending = true;
  if (pt->n_net)
    hipLaunchKernelGGL(partner_gather_nets_kernel<1>, dim3((pt->n_all + kPartnerGatherThreads - 1) / kPartnerGatherThreads), dim3(kPartnerGatherThreads), 0, s, gn);
  else
    hipLaunchKernelGGL(partner_gather_kernel<1>, dim3((M + kPartnerGatherThreads - 1) / kPartnerGatherThreads), dim3(kPartnerGatherThreads), 0, s, pt->g);
  HIP_TRY(hipGetLastError());
  for (int k = 0; k < pt->n_net; ++k) {   // a net's state rows of the games that just ended
    const PartnerNet& pn = pt->nets[k];
    CK(hsad_zero_state_rows(pn.h[nnxt], pn.c[nnxt], pn.fused ? pn.h16[nnxt] : nullptr, pt->g.c_terminal + pn.off, pn.L, pn.n, pn.H, 1, stream));
  }
  pt->net_cur = nnxt;
  ac->num_act += M;
  ac->step_no += 1;
  return actor_tail(ac, stream, nxt, pt->g.c_reward, pt->g.c_terminal, 1);
}

}  // namespace

// csrc/hsad_agent.hip
extern "C" int hsad_internal_net_dims(const hsad_r2d2_net* n, int* in_dim, int* hid_dim, int* num_action, int* num_lstm_layer, int* device);

extern "C" int hsad_actor_create_partnered(hsad_env* env, hsad_r2d2_net* online, hsad_r2d2_net* target, hsad_replay* replay,
                                           const hsad_actor_config* cfg, const hsad_actor_io* io, const hsad_actor_partners* partners,
                                           hsad_actor** out) {
  return hsad_actor_create_partnered_nets(env, online, target, replay, cfg, io, partners, nullptr, out);
}

extern "C" int hsad_actor_create_partnered_nets(hsad_env* env, hsad_r2d2_net* online, hsad_r2d2_net* target, hsad_replay* replay,
                                                const hsad_actor_config* cfg, const hsad_actor_io* io, const hsad_actor_partners* partners,
                                                const hsad_actor_net_partners* np, hsad_actor** out) {
  if (!env || !cfg || !partners || !out) return xfail(HSAD_ERR_INVALID, "actor_create_partnered: null argument");
  if (!partners->rows || !partners->seat_bot || (partners->n_bot > 0 && (!partners->rules || !partners->n_rules)))
    return xfail(HSAD_ERR_INVALID, "actor_create_partnered: null array in hsad_actor_partners");
  if (np && (!np->nets || !np->seat_net)) return xfail(HSAD_ERR_INVALID, "actor_create_partnered: null array in hsad_actor_net_partners");
  const int G = hsad_env_num_games(env), P = hsad_env_num_players(env), M = partners->M;
  const int F_env = hsad_env_feature_size(env), A_env = hsad_env_num_action(env);
  const int n_net = np ? np->n_net : 0;
  int32_t net_F[HSAD_PARTNER_MAX_NETS] = {}, net_A[HSAD_PARTNER_MAX_NETS] = {};
  int net_H[HSAD_PARTNER_MAX_NETS] = {}, net_L[HSAD_PARTNER_MAX_NETS] = {}, net_dev[HSAD_PARTNER_MAX_NETS] = {};
  if (n_net >= 1 && n_net <= HSAD_PARTNER_MAX_NETS) {   // (outside: the verdict refuses n_net before it reads a net's dimensions)
    for (int k = 0; k < n_net; ++k) {
      if (!np->nets[k]) return xfail(HSAD_ERR_INVALID, "actor_create_partnered: nets[%d] is NULL", k);
      int f = 0, a = 0;
      CK(hsad_internal_net_dims(np->nets[k], &f, &net_H[k], &a, &net_L[k], &net_dev[k]));
      net_F[k] = f;
      net_A[k] = a;
    }
  }
  const PartnerVerdict v = partner_layout_verdict_nets(G, P, cfg->hand_size, cfg->vdn, partners->rows, M, partners->rules, partners->n_rules,
                                                       partners->n_bot, partners->seat_bot, F_env, A_env, n_net, net_F, net_A,
                                                       np ? np->seat_net : nullptr);
  if (v.code != PT_OK) {
    char why[256];
    partner_verdict_text_nets(v, G, P, partners->n_bot, n_net, F_env, A_env, why, sizeof(why));
    return xfail(HSAD_ERR_INVALID, "actor_create_partnered: %s", why);
  }
  int dev_now = 0;
  (void)hipGetDevice(&dev_now);
  for (int k = 0; k < n_net; ++k) {   // handle identity: two act calls never share a net's workspace
    if (np->nets[k] == online || np->nets[k] == target)
      return xfail(HSAD_ERR_INVALID, "actor_create_partnered: nets[%d] is the %s net of this actor: a partner is a handle of its own (make a copy)", k,
                   np->nets[k] == online ? "online" : "target");
    for (int j = 0; j < k; ++j)
      if (np->nets[j] == np->nets[k])
        return xfail(HSAD_ERR_INVALID, "actor_create_partnered: nets[%d] is the same handle as nets[%d]: a partner is a handle of its own (make a copy)", k, j);
    if (net_dev[k] != dev_now)
      return xfail(HSAD_ERR_INVALID, "actor_create_partnered: nets[%d] lives on device %d, the actor on device %d", k, net_dev[k], dev_now);
  }
  auto* pt = new PartnerSeats();
  int G_env = 0;
  int rc = hsad_internal_env_rulebot_view(env, &pt->planes, &pt->act_count, &G_env, &pt->Gpad, &pt->ru);
  hsad_actor* ac = nullptr;
  if (!rc) rc = actor_create_rows(env, online, target, replay, cfg, io, M, &ac);   // the other refusals of hsad_actor_create
  if (rc) {
    partner_free(pt);
    return rc;
  }
  ac->partner = pt;   // from here on hsad_actor_destroy frees pt
  const int Fp = ac->Fp, A = ac->A, pw64 = (ac->F + 63) / 64;
  const size_t N = (size_t)G * P;
  if ((Fp & 7) || ((uintptr_t)io->priv_s_bf16 & 15u)) {
    hsad_actor_destroy(ac);
    return xfail(HSAD_ERR_INVALID, "actor_create_partnered: the bf16 observation rows must be 16-byte aligned and a multiple of 8 values long");
  }
  memset(&pt->bots, 0, sizeof(pt->bots));
  for (int b = 0; b < partners->n_bot; ++b) {
    const hsad_rule* r = partners->rules + (size_t)b * HSAD_RULE_MAX_RULES;
    for (int j = 0; j < partners->n_rules[b]; ++j) pt->bots.table[b * HSAD_RULE_MAX_RULES + j] = rb_pack(r[j].code, r[j].k);
    pt->bots.table[HSAD_RULE_MAX_BOTS * HSAD_RULE_MAX_RULES + b] = (uint32_t)partners->n_rules[b];
  }
  pt->bots.n_bot = partners->n_bot;
  pt->bot_seed = partners->bot_seed;
  auto up = [](size_t b) { return (b + 255) & ~(size_t)255; };
  // the compact index space: the learner's M rows, then the rows of net 0, net 1, ... each in ascending order
  std::vector<int32_t> rows_all(partners->rows, partners->rows + M);
  size_t net_bytes = 0;
  pt->n_net = n_net;
  for (int k = 0; k < n_net; ++k) {
    PartnerNet& pn = pt->nets[k];
    pn.net = np->nets[k];
    pn.off = (int)rows_all.size();
    for (size_t r = 0; r < N; ++r)
      if (np->seat_net[r] == k) rows_all.push_back((int32_t)r);
    pn.n = (int)rows_all.size() - pn.off;
    pn.L = net_L[k];
    pn.H = net_H[k];
    pn.fused = pn.n >= 1024;
    const size_t nh = (size_t)pn.L * pn.n * pn.H;
    net_bytes += 2 * (2 * up(nh * 4) + up(nh * 2)) + up((size_t)pn.n * 4);
  }
  const size_t n_all = rows_all.size();
  pt->n_all = (int)n_all;
  const size_t total = up(n_all * 4) + up(N * 4) + up(n_all * Fp * 2) + up(n_all * A * 4) + up(M * 4) + up((size_t)M * pw64 * 8) +
                       2 * up(M * 8) + up(M * 4) + up(n_all) + 2 * up(N * 8) + (n_net ? 2 * up(n_all * 8) : 0) + net_bytes;
  if (hipMalloc((void**)&pt->arena, total) != hipSuccess) {
    hsad_actor_destroy(ac);
    return xfail(HSAD_ERR_NOMEM, "actor_create_partnered: hipMalloc of %zu bytes failed", total);
  }
  (void)hipMemset(pt->arena, 0, total);
  char* p = pt->arena;
  auto take = [&](size_t b) {
    char* r = p;
    p += up(b);
    return r;
  };
  PartnerGather& g = pt->g;
  int32_t* d_rows = (int32_t*)take(n_all * 4);
  pt->seat = (int32_t*)take(N * 4);
  g.rows = d_rows;
  g.M = M;
  g.P = P;
  g.obs16 = (const uint4*)io->priv_s_bf16;
  g.legal = io->legal_move;
  g.eps = io->eps;
  g.priv_bits = (const unsigned long long*)io->priv_bits;
  g.legal_bits = (const unsigned long long*)io->legal_bits;
  g.own_bits = (const unsigned long long*)io->own_bits;
  g.reward = io->reward;
  g.terminal = io->terminal;
  g.c_obs16 = (uint4*)take(n_all * Fp * 2);
  g.c_legal = (float*)take(n_all * A * 4);
  g.c_eps = (float*)take(M * 4);
  g.c_priv_bits = (unsigned long long*)take((size_t)M * pw64 * 8);
  g.c_legal_bits = (unsigned long long*)take(M * 8);
  g.c_own_bits = (unsigned long long*)take(M * 8);
  g.c_reward = (float*)take(M * 4);
  g.c_terminal = (uint8_t*)take(n_all);
  g.n_obs = Fp / 8;
  g.pw64 = pw64;
  g.pb_vec = (pw64 % 2 == 0) && !((uintptr_t)io->priv_bits & 15u);
  g.n_pb = g.pb_vec ? pw64 / 2 : pw64;
  g.A = A;
  g.lg_vec = (A % 4 == 0) && !((uintptr_t)io->legal_move & 15u);
  g.n_lg = g.lg_vec ? A / 4 : A;
  // the arena of hsad_actor_create holds a / greedy for the agent's rows: here the compact act output; the full [G, P] pair the env
  // steps with (hsad_actor_last_actions) lives in this arena
  pt->a_c = ac->a;
  pt->g_c = ac->greedy;
  ac->a = (int64_t*)take(N * 8);
  ac->greedy = (int64_t*)take(N * 8);
  if (n_net) {   // every act call's output in one pair of arrays: the learner's slice in front, as the sequence writer reads it
    pt->a_c = (int64_t*)take(n_all * 8);
    pt->g_c = (int64_t*)take(n_all * 8);
  }
  for (int k = 0; k < n_net; ++k) {   // (zeroed with the arena: the initial state)
    PartnerNet& pn = pt->nets[k];
    const size_t nh = (size_t)pn.L * pn.n * pn.H;
    for (int slot = 0; slot < 2; ++slot) {
      pn.h[slot] = (float*)take(nh * 4);
      pn.c[slot] = (float*)take(nh * 4);
      pn.h16[slot] = (void*)take(nh * 2);
    }
    pn.temp = (float*)take((size_t)pn.n * 4);
  }
  // seat[r] = -(e + 1) means "this row's action is entry e of the compact act output", for the learner's rows and the nets' alike
  std::vector<int32_t> seat(N);
  for (size_t r = 0; r < N; ++r) seat[r] = partners->seat_bot[r];
  for (size_t e = 0; e < n_all; ++e) seat[rows_all[e]] = -((int32_t)e + 1);
  if (hipMemcpy(d_rows, rows_all.data(), n_all * 4, hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(pt->seat, seat.data(), N * 4, hipMemcpyHostToDevice) != hipSuccess) {
    hsad_actor_destroy(ac);
    return xfail(HSAD_ERR_HIP, "actor_create_partnered: copying the seat layout to the device failed");
  }
  *out = ac;
  return 0;
}

extern "C" int hsad_actor_partner_state(hsad_actor* ac, int k, float** h, float** c, int32_t* n_rows) {
  if (!ac || !h || !c) return xfail(HSAD_ERR_INVALID, "actor_partner_state: null argument");
  const PartnerSeats* pt = ac->partner;
  if (!pt || k < 0 || k >= pt->n_net)
    return xfail(HSAD_ERR_INVALID, "actor_partner_state: net %d, the actor has %d network partners", k, pt ? pt->n_net : 0);
  *h = pt->nets[k].h[pt->net_cur];
  *c = pt->nets[k].c[pt->net_cur];
  if (n_rows) *n_rows = pt->nets[k].n;
  return 0;
}

extern "C" int hsad_actor_set_partner_temperature(hsad_actor* ac, int k, float tau) {
  if (!ac) return xfail(HSAD_ERR_INVALID, "actor_set_partner_temperature: null actor");
  PartnerSeats* pt = ac->partner;
  if (!pt || k < 0 || k >= pt->n_net)
    return xfail(HSAD_ERR_INVALID, "actor_set_partner_temperature: net %d, the actor has %d network partners", k, pt ? pt->n_net : 0);
  if (!(tau >= 0.f) || !std::isfinite(tau))
    return xfail(HSAD_ERR_INVALID, "actor_set_partner_temperature: the temperature must be finite and >= 0; got %g", (double)tau);
  PartnerNet& pn = pt->nets[k];
  // rare and host-side: wait for the steps that may still read the vector, then write it with a blocking copy
  const std::vector<float> v((size_t)pn.n, tau);
  if (hipDeviceSynchronize() != hipSuccess || hipMemcpy(pn.temp, v.data(), v.size() * 4, hipMemcpyHostToDevice) != hipSuccess)
    return xfail(HSAD_ERR_HIP, "actor_set_partner_temperature: writing the temperature vector failed");
  pn.tau = tau;
  return 0;
}
