// hsad_env_belief.inc — the exact belief over a hidden hand, and the sampler built on it: how many hands the viewer's card knowledge
// allows and with what per-slot marginals (hsad_env_hand_belief), and the rejection-free, stratifiable counterpart of
// hsad_env_determinize that turns a rank in [0, N) into a hand (hsad_env_determinize_exact); and the env side of the learned belief
// (hsad_belief_head.h): every seat's knowledge of its own hand (hsad_env_hand_knowledge) and the sampler that draws a hand from the
// exact belief tilted by a head's logits (hsad_env_determinize_belief; hsad_env_determinize_belief_worlds, appended at the end of
// the file, for a search env: logits by root game, the worlds of a game stratified per slot).  Textually part of hsad_env.hip, after
// hsad_env_search.inc: it uses that file's compat_mask, observe pass and SAD-section source as they are.  The integer arithmetic is
// hsad_hand_count.h, shared with the CPU suite.  Nothing here is reached by any other entry point.

#include "hsad_hand_count.h"
#include "hsad_belief_head.h"

namespace {

constexpr int kBeliefThreads = 128;   // >= 5 slots x 25 types

// the viewer's hand as the arithmetic wants it; false = the game is skipped
struct HandKnowledge {
  uint64_t pool;
  uint32_t cm[HC_MAX_SLOTS];
  uint32_t hw;
  int L;
};
__device__ __forceinline__ bool hand_knowledge(const EnvParams& ep, int g, int p, HandKnowledge* k) {
  const int P = ep.P;
  const uint32_t misc = GP(PL_MISC);
  if (p < 0 || p >= P || !misc_live(misc)) return false;
  const uint32_t hw = GP(PLH(p)), kcp = GP(PLKCP(p)), krp = GP(PLKRP(p));
  const int L = min((int)((hw >> 25) & 7u), HC_MAX_SLOTS);
  uint64_t pool = (uint64_t)GP(PL_DECK_LO) | ((uint64_t)GP(PL_DECK_HI) << 32);
  for (int i = 0; i < HC_MAX_SLOTS; ++i) {
    k->cm[i] = i < L ? compat_mask((kcp >> (5 * i)) & 31u, (krp >> (5 * i)) & 31u) : 0u;
    if (i < L) pool += (uint64_t)1 << (2 * ((hw >> (5 * i)) & 31u));
  }
  k->pool = pool;
  k->hw = hw;
  k->L = L;
  return true;
}

// ---- belief: one workgroup of 128 threads per game --------------------------------------------------------------------------------
// Threads 0..31 fill the table of subset sums in LDS (one set of slots each); thread i * 25 + t then evaluates num[i][t] = one count
// over the other slots with one card of type t removed, thread 127 the total; threads 0 .. 3H-1 sum the trinary classes from LDS.
// Thread k's counts_out store is word k of the game's [H, 25] block: consecutive lanes, consecutive words.  A skipped game's blocks
// are zeroed the same way.  The skip test depends on the game alone, so every barrier is uniform over the workgroup.
__global__ __launch_bounds__(kBeliefThreads) void env_hand_belief_kernel(EnvParams ep, const int32_t* __restrict__ viewer,
                                                                         int64_t* __restrict__ total_out, int64_t* __restrict__ counts_out,
                                                                         int64_t* __restrict__ trinary_out) {
  __shared__ HcTables s_tab;
  __shared__ int64_t s_num[HC_MAX_SLOTS * HC_TYPES];
  const int g = blockIdx.x;   // < G: the grid is G workgroups
  const int tid = threadIdx.x;
  const int H = ep.H;
  const int i = tid / HC_TYPES, t = tid - i * HC_TYPES;
  int64_t* counts = counts_out + (size_t)g * H * HC_TYPES;
  int64_t* tri = trinary_out ? trinary_out + (size_t)g * H * 3 : nullptr;
  HandKnowledge k;
  if (!hand_knowledge(ep, g, viewer[g], &k)) {
    if (tid < H * HC_TYPES) counts[tid] = 0;
    if (tri && tid < H * 3) tri[tid] = 0;
    if (tid == 0) total_out[g] = 0;
    return;
  }
  const uint32_t all = hc_all_slots(k.L);
  if (tid >= 1 && tid < HC_SUBSETS && !((uint32_t)tid & ~all)) {
    const uint32_t am = hc_and_mask(k.cm, (uint32_t)tid);
    s_tab.and_mask[tid] = am;
    s_tab.s[tid] = hc_weight(k.pool, am);
  }
  __syncthreads();
  int64_t num = 0;
  if (i < k.L) num = hc_marginal(s_tab.and_mask, s_tab.s, k.pool, k.cm, k.L, i, t);
  if (tid == kBeliefThreads - 1) total_out[g] = hc_count(s_tab.and_mask, s_tab.s, all, -1);
  if (tid < H * HC_TYPES) counts[tid] = num;
  if (!tri) return;
  if (tid < HC_MAX_SLOTS * HC_TYPES) s_num[tid] = num;
  __syncthreads();
  if (tid < H * 3) {
    const int slot = tid / 3, cls = tid - slot * 3;
    const uint32_t board = GP(PL_BOARD);
    int64_t sum = 0;
    for (int c = 0; c < 5; ++c) {
      const int fw = board_fw(board, c);
      for (int r = 0; r < 5; ++r) sum += hc_trinary_class(r, fw) == cls ? s_num[slot * HC_TYPES + c * 5 + r] : 0;
    }
    tri[tid] = sum;
  }
}

// ---- exact determinise: one thread per game, the shape of env_determinize_kernel ---------------------------------------------------
// N from the tables of the pool, the rank (given, or drawn from the world's stratum with two words of hash stream 65), the unranking.
// A game left alone -- skipped, rank or stratum out of range, N = 0 -- gets rank_out = -1 and sel = -1 (the observe pass passes it by).
__global__ void env_determinize_exact_kernel(EnvParams ep, const int32_t* __restrict__ viewer, const int64_t* __restrict__ key, uint64_t seed,
                                             const int32_t* __restrict__ stratum, int n_strata, const int64_t* __restrict__ rank_in,
                                             int64_t* __restrict__ rank_out, int32_t* __restrict__ sel) {
  const int g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= ep.G) return;
  int64_t rank = -1;
  HandKnowledge k;
  if (hand_knowledge(ep, g, viewer[g], &k)) {
    const int p = viewer[g];
    const int64_t N = hc_total(k.pool, k.cm, k.L);
    int64_t r = -1;
    if (rank_in) {
      r = rank_in[g];
    } else {
      const int w = stratum ? stratum[g] : 0;
      if (w >= 0 && w < n_strata && N > 0) {
        const uint64_t k64 = (uint64_t)key[g];
        const uint64_t u = ((uint64_t)policy_hash(seed, k64, 0ull, 65ull) << 32) | (uint64_t)policy_hash(seed, k64, 1ull, 65ull);
        r = hc_stratum_rank(N, (int64_t)w, (int64_t)n_strata, u);
      }
    }
    uint32_t cards = 0;
    uint64_t q = 0;
    if (r >= 0 && r < N && hc_unrank(k.pool, k.cm, k.L, r, &cards, &q)) {
      const uint32_t low = k.L >= 5 ? 0x1ffffffu : ((1u << (5 * k.L)) - 1u);
      GP(PLH(p)) = (k.hw & ~low) | cards;
      GP(PL_DECK_LO) = (uint32_t)q;
      GP(PL_DECK_HI) = (uint32_t)(q >> 32);
      rank = r;
    }
  }
  if (rank_out) rank_out[g] = rank;
  sel[g] = rank >= 0 ? g : -1;
}

// ---- the knowledge of every seat, as the learned belief's dataset stores it: one thread per (game, seat) ---------------------------
// pool / compat are hand_knowledge's (what env_hand_belief_kernel counts with for that viewer), cards the seat's true hand; a game
// that is not live gets zeros and -1.  Reads the state only.
__global__ void env_hand_knowledge_kernel(EnvParams ep, int64_t* __restrict__ pool_out, int32_t* __restrict__ compat_out,
                                          int32_t* __restrict__ cards_out) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= ep.G * ep.P) return;
  const int g = r / ep.P, p = r - g * ep.P, H = ep.H;
  HandKnowledge k;
  const bool live = hand_knowledge(ep, g, p, &k);
  pool_out[r] = live ? (int64_t)k.pool : 0;
  for (int i = 0; i < H; ++i) {
    const bool occ = live && i < k.L;
    compat_out[(size_t)r * H + i] = occ ? (int32_t)k.cm[i] : 0;
    cards_out[(size_t)r * H + i] = occ ? (int32_t)((k.hw >> (5 * i)) & 31u) : -1;
  }
}

// ---- learned-belief determinise: one thread per game, the shape of env_determinize_exact_kernel ------------------------------------
// The hand of viewer[g] becomes bh_row's sample (csrc/hsad_belief_head.h, sample mode) under the game's logits row, slot i drawing
// with the policy hash of (seed, key[g], i) on stream 66; the deck counts become the pool the sample leaves.  A game left alone --
// skipped, or a row the sampler refuses (non-finite logits) -- gets status 0, logp 0 and sel = -1.
__global__ void env_determinize_belief_kernel(EnvParams ep, const int32_t* __restrict__ viewer, const float* __restrict__ logits, int ldz,
                                              const int64_t* __restrict__ key, uint64_t seed, float* __restrict__ logp_out,
                                              int32_t* __restrict__ status_out, int32_t* __restrict__ sel) {
  const int g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= ep.G) return;
  int status = 0;
  float logp = 0.f;
  HandKnowledge k;
  if (hand_knowledge(ep, g, viewer[g], &k)) {
    const int p = viewer[g];
    const uint64_t k64 = (uint64_t)key[g];
    uint32_t u[HC_MAX_SLOTS];
    for (int i = 0; i < HC_MAX_SLOTS; ++i) u[i] = policy_hash(seed, k64, (uint64_t)i, 66ull);
    const bh_row_out r = bh_row(logits + (size_t)g * ldz, k.pool, k.cm, nullptr, u, k.L, ep.H, 0.f, false, 0, [](int, float) {});
    if (!r.bad) {
      const uint32_t low = k.L >= 5 ? 0x1ffffffu : ((1u << (5 * k.L)) - 1u);
      GP(PLH(p)) = (k.hw & ~low) | r.hand;
      GP(PL_DECK_LO) = (uint32_t)r.q;
      GP(PL_DECK_HI) = (uint32_t)(r.q >> 32);
      status = 1;
      logp = -r.nll;
    }
  }
  if (logp_out) logp_out[g] = logp;
  if (status_out) status_out[g] = status;
  sel[g] = status ? g : -1;
}

}  // namespace

extern "C" {

int hsad_env_hand_knowledge(hsad_env* e, int64_t* pool_out, int32_t* compat_out, int32_t* cards_out, void* stream) {
  if (!e || !pool_out || !compat_out || !cards_out) return set_error(HSAD_ERR_INVALID, "null argument");
  if (e->ep.H > HC_MAX_SLOTS) return set_error(HSAD_ERR_INVALID, "hsad_env_hand_knowledge: hands of more than 5 slots");
  const int n = e->ep.G * e->ep.P;
  hipLaunchKernelGGL(env_hand_knowledge_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, e->ep, pool_out, compat_out, cards_out);
  HIP_TRY(hipGetLastError());
  return HSAD_OK;
}

int hsad_env_determinize_belief(hsad_env* e, const int32_t* viewer, const float* logits, int ldz, const int64_t* key, uint64_t seed,
                                float* logp_out, int32_t* status_out, void* stream) {
  if (!e || !viewer || !logits || !key) return set_error(HSAD_ERR_INVALID, "null argument");
  if (e->ep.H > HC_MAX_SLOTS) return set_error(HSAD_ERR_INVALID, "hsad_env_determinize_belief: hands of more than 5 slots");
  if (ldz < e->ep.H * HC_TYPES) return set_error(HSAD_ERR_INVALID, "hsad_env_determinize_belief: ldz must be at least 25 logits per slot of the hand");
  if (!e->bound) return set_error(HSAD_ERR_STATE, "hsad_env_bind_outputs must be called first");
  ObserveArgs oa;
  if (!sad_source(e, &oa) && e->ep.sad)
    return set_error(HSAD_ERR_INVALID, "hsad_env_determinize_belief: sad = 1 needs the env's own observation rows (float32 or bit words)");
  if (!e->d_sel) {
    HIP_TRY(hipSetDevice(e->device));
    HIP_TRY(hipMalloc((void**)&e->d_sel, sizeof(int32_t) * (size_t)e->ep.Gpad));
  }
  oa.sel = e->d_sel;
  oa.sel_limit = e->ep.G;
  hipLaunchKernelGGL(env_determinize_belief_kernel, dim3((e->ep.G + 63) / 64), dim3(64), 0, (hipStream_t)stream, e->ep, viewer, logits, ldz, key,
                     seed, logp_out, status_out, e->d_sel);
  HIP_TRY(hipGetLastError());
  return launch_observe(e, oa, (hipStream_t)stream);
}

int hsad_env_hand_belief(hsad_env* e, const int32_t* viewer, int64_t* total_out, int64_t* counts_out, int64_t* trinary_out, void* stream) {
  if (!e || !viewer || !total_out || !counts_out) return set_error(HSAD_ERR_INVALID, "null argument");
  if (e->ep.H > HC_MAX_SLOTS) return set_error(HSAD_ERR_INVALID, "hsad_env_hand_belief: hands of more than 5 slots");
  hipLaunchKernelGGL(env_hand_belief_kernel, dim3(e->ep.G), dim3(kBeliefThreads), 0, (hipStream_t)stream, e->ep, viewer, total_out,
                     counts_out, trinary_out);
  HIP_TRY(hipGetLastError());
  return HSAD_OK;
}

int hsad_env_determinize_exact(hsad_env* e, const int32_t* viewer, const int64_t* key, uint64_t seed, const int32_t* stratum, int n_strata,
                               const int64_t* rank_in, int64_t* rank_out, void* stream) {
  if (!e || !viewer || (!key && !rank_in)) return set_error(HSAD_ERR_INVALID, "null argument");
  if (n_strata < 1 || n_strata > (1 << 20)) return set_error(HSAD_ERR_INVALID, "hsad_env_determinize_exact: n_strata must be in [1, 2^20]");
  if (e->ep.H > HC_MAX_SLOTS) return set_error(HSAD_ERR_INVALID, "hsad_env_determinize_exact: hands of more than 5 slots");
  if (!e->bound) return set_error(HSAD_ERR_STATE, "hsad_env_bind_outputs must be called first");
  ObserveArgs oa;
  if (!sad_source(e, &oa) && e->ep.sad)
    return set_error(HSAD_ERR_INVALID, "hsad_env_determinize_exact: sad = 1 needs the env's own observation rows (float32 or bit words)");
  if (!e->d_sel) {
    HIP_TRY(hipSetDevice(e->device));
    HIP_TRY(hipMalloc((void**)&e->d_sel, sizeof(int32_t) * (size_t)e->ep.Gpad));
  }
  oa.sel = e->d_sel;
  oa.sel_limit = e->ep.G;
  hipLaunchKernelGGL(env_determinize_exact_kernel, dim3((e->ep.G + 255) / 256), dim3(256), 0, (hipStream_t)stream, e->ep, viewer, key, seed,
                     stratum, n_strata, rank_in, rank_out, e->d_sel);
  HIP_TRY(hipGetLastError());
  return launch_observe(e, oa, (hipStream_t)stream);
}

}  // extern "C"

// ---- learned-belief determinise for a search env: logits by root game, the worlds of a game stratified per slot --------------------
// env_determinize_belief_kernel's shape (one thread per game, 64 games per workgroup) and bh_row call; what differs is where the row
// and the uniforms come from: game g reads logits row row[g] (NULL: g), and its slot uniforms are hsad_belief_world.h's for world
// world[g] of n_worlds of the root game group[g] (hash stream 67).  A game left alone -- skipped, row or world out of range, a row
// the sampler refuses -- gets status 0, logp = logp0 = 0 and sel = -1.
#include "hsad_belief_world.h"

namespace {

__global__ __launch_bounds__(64) void env_determinize_belief_worlds_kernel(EnvParams ep, const int32_t* __restrict__ viewer,
                                                                           const float* __restrict__ logits, int ldz, int n_rows,
                                                                           const int32_t* __restrict__ row, const int64_t* __restrict__ group,
                                                                           const int32_t* __restrict__ world, int n_worlds, uint64_t seed,
                                                                           float* __restrict__ logp_out, float* __restrict__ logp0_out,
                                                                           int32_t* __restrict__ status_out, int32_t* __restrict__ sel) {
  const int g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= ep.G) return;
  int status = 0;
  float logp = 0.f, logp0 = 0.f;
  HandKnowledge k;
  const int zr = row ? row[g] : g;
  if (zr >= 0 && zr < n_rows && hand_knowledge(ep, g, viewer[g], &k)) {
    const int p = viewer[g];
    const uint64_t k64 = (uint64_t)group[g];
    uint32_t u[HC_MAX_SLOTS];
    if (bw_uniforms([seed, k64](uint64_t c) { return policy_hash(seed, k64, c, (uint64_t)BW_STREAM); }, (int64_t)n_worlds, (int64_t)world[g], u,
                    nullptr)) {
      const bh_row_out r = bh_row(logits + (size_t)zr * ldz, k.pool, k.cm, nullptr, u, k.L, ep.H, 0.f, false, 0, [](int, float) {});
      if (!r.bad) {
        const uint32_t low = k.L >= 5 ? 0x1ffffffu : ((1u << (5 * k.L)) - 1u);
        GP(PLH(p)) = (k.hw & ~low) | r.hand;
        GP(PL_DECK_LO) = (uint32_t)r.q;
        GP(PL_DECK_HI) = (uint32_t)(r.q >> 32);
        status = 1;
        logp = -r.nll;
        logp0 = -r.nll0;
      }
    }
  }
  if (logp_out) logp_out[g] = logp;
  if (logp0_out) logp0_out[g] = logp0;
  if (status_out) status_out[g] = status;
  sel[g] = status ? g : -1;
}

}  // namespace

extern "C" int hsad_env_determinize_belief_worlds(hsad_env* e, const int32_t* viewer, const float* logits, int ldz, int n_rows, const int32_t* row,
                                                  const int64_t* group, const int32_t* world, int n_worlds, uint64_t seed, float* logp_out,
                                                  float* logp0_out, int32_t* status_out, void* stream) {
  if (!e || !viewer || !logits || !group || !world) return set_error(HSAD_ERR_INVALID, "null argument");
  if (e->ep.H > HC_MAX_SLOTS) return set_error(HSAD_ERR_INVALID, "hsad_env_determinize_belief_worlds: hands of more than 5 slots");
  if (ldz < e->ep.H * HC_TYPES)
    return set_error(HSAD_ERR_INVALID, "hsad_env_determinize_belief_worlds: ldz must be at least 25 logits per slot of the hand");
  if (n_rows < 1 || (!row && n_rows < e->ep.G))
    return set_error(HSAD_ERR_INVALID, "hsad_env_determinize_belief_worlds: n_rows must be >= 1, and >= the env's games without a row index");
  if (n_worlds < 1 || n_worlds > (int)BW_MAX_WORLDS)
    return set_error(HSAD_ERR_INVALID, "hsad_env_determinize_belief_worlds: n_worlds must be in [1, 2^20]");
  if (!e->bound) return set_error(HSAD_ERR_STATE, "hsad_env_bind_outputs must be called first");
  ObserveArgs oa;
  if (!sad_source(e, &oa) && e->ep.sad)
    return set_error(HSAD_ERR_INVALID, "hsad_env_determinize_belief_worlds: sad = 1 needs the env's own observation rows (float32 or bit words)");
  if (!e->d_sel) {
    HIP_TRY(hipSetDevice(e->device));
    HIP_TRY(hipMalloc((void**)&e->d_sel, sizeof(int32_t) * (size_t)e->ep.Gpad));
  }
  oa.sel = e->d_sel;
  oa.sel_limit = e->ep.G;
  hipLaunchKernelGGL(env_determinize_belief_worlds_kernel, dim3((e->ep.G + 63) / 64), dim3(64), 0, (hipStream_t)stream, e->ep, viewer, logits, ldz,
                     n_rows, row, group, world, n_worlds, seed, logp_out, logp0_out, status_out, e->d_sel);
  HIP_TRY(hipGetLastError());
  return launch_observe(e, oa, (hipStream_t)stream);
}
