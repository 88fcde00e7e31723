// hsad_env_search.inc — the env as a simulator for test-time search: fork games between env batches, resample a hidden hand from
// the card knowledge, rebuild the observations of a changed state, play games out at random.  Textually part of hsad_env.hip
// (included at its end: the kernels below use its state planes, its game logic and its row builder as they are).
//
// Nothing here is reached by reset / step / rollout: the four kernels are separate launches, and the existing modes 0-3 of
// env_kernel are compiled from unchanged code.

namespace {

// ---- observe: build_rows + the row stream for chosen games, no game logic -----------------------------------------------------
// Game g of the launch's env is observed iff 0 <= sel[g] < sel_limit.  The SAD last-action section (the greedy record exists only
// in LDS while a step runs, no state plane holds it) is copied from rows sel[g] * P + p of the source observation: bit words when
// the source has them, float32 otherwise.  For hsad_env_determinize the source is the env itself (sel[g] = g): a workgroup reads
// its own games' rows before the barrier and rewrites them after it.
struct ObserveArgs {
  const int32_t* sel;
  int sel_limit;
  const unsigned long long* sad_bits;  // [*, sad_pw64] or NULL
  int sad_pw64;
  const float* sad_f32;                // [*, F] (used when sad_bits is NULL); both NULL: an all-zero section, as after a reset
  const unsigned long long* sad_words; // [*] the section itself, one word per row (hsad_env_sad_section); wins over the other two
};

__device__ __forceinline__ uint64_t sad_section_of(const EnvParams& ep, const ObserveArgs& oa, size_t row) {
  const uint64_t mask = (1ull << ep.LAL) - 1ull;   // LAL <= 61
  if (oa.sad_words) return oa.sad_words[row] & mask;
  if (oa.sad_bits) {
    const unsigned long long* r = oa.sad_bits + row * (size_t)oa.sad_pw64;
    const int w = ep.F0 >> 6, sh = ep.F0 & 63;
    uint64_t v = r[w] >> sh;
    if (sh && w + 1 < oa.sad_pw64) v |= r[w + 1] << (64 - sh);
    return v & mask;
  }
  if (!oa.sad_f32) return 0ull;
  const float* r = oa.sad_f32 + row * (size_t)ep.F + ep.F0;
  uint64_t v = 0;
  for (int i = 0; i < ep.LAL; ++i) v |= (uint64_t)(r[i] != 0.f ? 1u : 0u) << i;
  return v;
}

// Layout: one workgroup per gpw games, the LDS of env_kernel's step (planes | obs | legal | own bit rows).  Wave 0 stages the
// planes while the others clear the rows; all waves build the chosen games' rows (observers strided over the waves, as in
// env_body); then the chosen games are dealt round-robin to the waves, and a wave streams its games' rows -- and, with
// knowledge_mode 1, fixes up their V0-belief section behind its own stores -- the way the reset kernel does for restarted games.
// A game that was never started gets all-zero rows and masks: what a freshly created env holds.
template <int TP, int TH, bool V>
__global__ __launch_bounds__(kEnvThreads) void env_observe_kernel(EnvParams ep, ObserveArgs oa) {
  extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
  uint32_t* s_st = smem;
  uint32_t* s_obs = s_st + ep.npl * kWave;
  uint32_t* s_legal = s_obs + ep.obs_words;
  uint32_t* s_own = s_legal + ep.legal_words;
  const int tid = threadIdx.x;
  const int lane = tid & (kWave - 1);
  const int wave = tid >> 6;
  const int nthreads = ep.nthreads, nwaves = nthreads >> 6;
  const int g0 = blockIdx.x * ep.gpw;
  const int g = g0 + lane;
  const bool valid = lane < ep.gpw && g < ep.G;
  const int P = TP ? TP : ep.P, H = TH ? TH : ep.H;
  const int src = valid ? oa.sel[g] : -1;
  const bool chosen = valid && src >= 0 && src < oa.sel_limit;
  const uint64_t todo = __ballot(chosen);
  if (todo == 0ull) return;   // the same 64 games in every wave: uniform over the workgroup
  if (wave == 0) {
    stage_planes(ep, s_st, lane, g);
  } else {
    clear_rows(ep, s_obs, tid - kWave, nthreads - kWave);
  }
  __syncthreads();
  const uint32_t misc = ST(PL_MISC);
  if (chosen && misc_started(misc)) {
    build_rows<TP, TH, V>(ep, s_st, lane, g, s_obs, s_legal, s_own, 0u, wave, nwaves);
    if (ep.sad)
      for (int p = wave; p < P; p += nwaves)
        or_bits64(s_obs, (uint32_t)(lane * P + p) * (uint32_t)ep.F + (uint32_t)ep.F0, sad_section_of(ep, oa, (size_t)src * P + p));
  } else if (chosen && wave == 0) {
    for (int p = 0; p < P; ++p) {
      ep.legal_bits[(size_t)g * P + p] = 0ull;
      if (ep.legal_out) ep.legal_out[(size_t)g * P + p] = 0ull;
      if (ep.own_bits) ep.own_bits[(size_t)g * P + p] = 0ull;
    }
  }
  __syncthreads();
  const size_t PF = (size_t)P * ep.F, PA = (size_t)P * ep.A, PO = (size_t)P * 3 * H;
  uint64_t rest = todo, mine = 0ull;
  for (int k = 0; rest; ++k) {
    const int lg = __builtin_ctzll(rest);
    rest &= rest - 1;
    if (k % nwaves != wave) continue;
    mine |= 1ull << lg;
    if (ep.obs_f32) stream_bits_f32(s_obs, (uint32_t)(lg * PF), ep.priv_s + (size_t)(g0 + lg) * PF, (uint32_t)PF, lane);
    stream_rows_packed(ep, s_obs, lg * P, P, (size_t)(g0 + lg) * P, lane, kWave);
    stream_bits_f32(s_legal, (uint32_t)(lg * PA), ep.legal + (size_t)(g0 + lg) * PA, (uint32_t)PA, lane);
    stream_bits_f32(s_own, (uint32_t)(lg * PO), ep.own + (size_t)(g0 + lg) * PO, (uint32_t)PO, lane);
  }
  if (chosen && wave == 0) {
    for (int p = 0; p < P; ++p) ep.eps[(size_t)g * P + p] = __uint_as_float(ST(PLEPS(p)));
    ep.reward[g] = 0.f;
    ep.terminal[g] = (uint8_t)misc_term(misc);
  }
  if (ep.kmode == 1) v0_fixup<V>(ep, s_st, s_obs, mine, g0, lane);
}

// ---- the SAD section of the env's current rows, one word per (game, seat) row: what a log keeps of an observation ---------------
__global__ void env_sad_section_kernel(EnvParams ep, ObserveArgs oa, unsigned long long* __restrict__ out) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= ep.G * ep.P) return;
  out[r] = ep.sad ? sad_section_of(ep, oa, (size_t)r) : 0ull;
}

// ---- fork: dst game j becomes src game src_index[j] -----------------------------------------------------------------------------
// One wave per destination game: its lanes copy the planes, the 624 generator words and the deck-history row.  With seeds the
// generator is seeded the way init_game seeds it (std::mt19937(seeds[j]): a serial recurrence, lane 0) and the draw counter and
// the look-ahead are emptied.
__global__ void env_fork_kernel(EnvParams d, EnvParams s, const int32_t* __restrict__ src_index, const int32_t* __restrict__ seeds,
                                int copy_dh) {
  const int lane = threadIdx.x & (kWave - 1);
  const int j = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (j >= d.G) return;
  const int si = src_index[j];
  if (si == -1) return;
  if (si < 0 || si >= s.G) {
    if (lane == 0) log_error(d, j, 4);
    return;
  }
  for (int pl = lane; pl < d.npl; pl += kWave) {
    uint32_t v = s.planes[(size_t)pl * s.Gpad + si];
    if (seeds) {
      if (pl == PL_DRAWS || pl == PL_LA0 || pl == PL_LA1) v = 0u;
      if (pl == PL_MISC) v &= ~(3u << 22);
    }
    d.planes[(size_t)pl * d.Gpad + j] = v;
  }
  if (lane == 0) d.act_count[j] = s.act_count[si];
  if (copy_dh && lane < 52) d.deck_hist[(size_t)j * 52 + lane] = s.deck_hist[(size_t)si * 52 + lane];
  uint32_t* mt = d.mt + (size_t)j * kMtN;
  if (!seeds) {
    const uint32_t* ms = s.mt + (size_t)si * kMtN;
    for (int k = lane; k < kMtN; k += kWave) mt[k] = ms[k];
  } else if (lane == 0) {
    uint32_t x = (uint32_t)seeds[j];
    mt[0] = x;
    for (int i = 1; i < kMtN; ++i) {
      x = 1812433253u * (x ^ (x >> 30)) + (uint32_t)i;
      mt[i] = x;
    }
  }
}

// ---- determinise: resample the viewer's hand uniformly from the hands its card knowledge allows -----------------------------------
// Slot-wise proposal from the shrinking pool (probability prod q_i / Z_i) thinned by prod Z_i / Zmax_i (Z_i <= Zmax_i: the pool only
// shrinks), so an accepted hand has probability proportional to prod q_i, the product of the falling counts: uniform over the
// assignments of physical unseen cards that agree with the masks.  All products stay below 2^61 (Z <= 50, five slots, u < 2^32).
__device__ __forceinline__ uint32_t compat_mask(uint32_t cp, uint32_t rp) {   // bit t = colour * 5 + rank
  uint32_t m = 0;
#pragma unroll
  for (int c = 0; c < 5; ++c) m |= ((cp >> c) & 1u) ? (rp << (5 * c)) : 0u;
  return m;
}
__device__ __forceinline__ uint32_t pool_weight(uint64_t q, uint32_t cm) {
  uint32_t z = 0;
#pragma unroll
  for (int t = 0; t < 25; ++t) z += ((cm >> t) & 1u) ? cnt2(q, t) : 0u;
  return z;
}

__global__ void env_determinize_kernel(EnvParams ep, const int32_t* __restrict__ viewer, const int64_t* __restrict__ key, uint64_t seed,
                                       int32_t* __restrict__ tries_out, int32_t* __restrict__ sel) {
  const int g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= ep.G) return;
  const int P = ep.P;
  const int p = viewer[g];
  const uint32_t misc = GP(PL_MISC);
  int tries = 0;
  bool changed = false;
  if (p >= 0 && p < P && misc_live(misc)) {
    const uint32_t hw = GP(PLH(p)), kcp = GP(PLKCP(p)), krp = GP(PLKRP(p));
    const int L = (hw >> 25) & 7;
    const uint64_t k64 = (uint64_t)key[g];
    uint64_t pool = (uint64_t)GP(PL_DECK_LO) | ((uint64_t)GP(PL_DECK_HI) << 32);
    for (int i = 0; i < L; ++i) pool += (uint64_t)1 << (2 * ((hw >> (5 * i)) & 31u));
    uint64_t zmax = 1;
    for (int i = 0; i < L; ++i) zmax *= pool_weight(pool, compat_mask((kcp >> (5 * i)) & 31u, (krp >> (5 * i)) & 31u));
    tries = -1;
    for (int t = 0; t < 32 && !changed; ++t) {
      uint64_t q = pool, zprod = 1;
      uint32_t cards = 0;
      bool ok = true;
      for (int i = 0; i < L && ok; ++i) {
        const uint32_t cm = compat_mask((kcp >> (5 * i)) & 31u, (krp >> (5 * i)) & 31u);
        const uint32_t Z = pool_weight(q, cm);
        if (Z == 0u) {
          ok = false;
          break;
        }
        const uint32_t h = policy_hash(seed, k64, (uint64_t)(t * 8 + i), 64ull);
        const uint32_t k = (uint32_t)(((uint64_t)h * Z) >> 32);
        uint32_t run = 0;
        int card = -1;
        for (int c = 0; c < 25; ++c) {
          run += ((cm >> c) & 1u) ? cnt2(q, c) : 0u;
          if (card < 0 && run > k) card = c;
        }
        q -= (uint64_t)1 << (2 * card);
        zprod *= Z;
        cards |= (uint32_t)card << (5 * i);
      }
      if (!ok) continue;
      const uint64_t u = policy_hash(seed, k64, (uint64_t)(t * 8 + 7), 64ull);
      if (u * zmax < (zprod << 32)) {
        const uint32_t low = L >= 5 ? 0x1ffffffu : ((1u << (5 * L)) - 1u);
        GP(PLH(p)) = (hw & ~low) | cards;
        GP(PL_DECK_LO) = (uint32_t)q;
        GP(PL_DECK_HI) = (uint32_t)(q >> 32);
        tries = t + 1;
        changed = true;
      }
    }
  }
  if (tries_out) tries_out[g] = tries;
  sel[g] = changed ? g : -1;
}

// ---- rewind: back to a fresh deal whose cards are the script's ----------------------------------------------------------------------
// One thread per game.  A game with count > 0 that is started and whose script is a legal deal order (count in [P * H, deck], every
// card a type the full deck still holds after the cards before it) is put back to what a reset leaves, with the hands dealt from
// script[0 .. P * H) in deal_one's order (seat 0's H cards first); its script row and count move into the env's own buffers, which
// the scripted step reads.  What reset drew from the generator stays: eps, colour permutations, generator words, draw counter,
// look-ahead, last score, policy counter.  A bad script is logged (code 5) and the game left alone; sel[g] = g for the rewound
// games (the observe pass that follows rewrites their rows), -1 otherwise.
__global__ void env_rewind_kernel(EnvParams ep, DealScript own, const uint8_t* __restrict__ script, const int32_t* __restrict__ count,
                                  int32_t* __restrict__ sel) {
  const int g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= ep.G) return;
  sel[g] = -1;
  const int n = count[g];
  if (n <= 0) return;
  const int P = ep.P, H = ep.H;
  const uint32_t misc = GP(PL_MISC);
  if (!misc_started(misc)) return;   // never started: reset has drawn no eps and no permutation to keep
  const uint8_t* sc = script + (size_t)g * 52;
  bool ok = n >= P * H && n <= ep.deck_max;
  uint64_t pool = ep.deck_full, deck = ep.deck_full;
  for (int i = 0; ok && i < n; ++i) {
    const int t = sc[i];
    if (t >= 25 || cnt2(pool, t) == 0u) {
      ok = false;
      break;
    }
    pool -= (uint64_t)1 << (2 * t);
    if (i + 1 == P * H) deck = pool;
  }
  if (!ok) {
    log_error(ep, g, 5);
    return;
  }
  for (int i = 0; i < 52; ++i) own.cards[(size_t)g * 52 + i] = i < n ? sc[i] : (uint8_t)0;
  own.count[g] = n;
  if (ep.track_dh)
    for (int i = 0; i < P * H; ++i) ep.deck_hist[(size_t)g * 52 + i] = sc[i];
  const uint32_t cmask = (1u << ep.nC) - 1u, rmask = (1u << ep.nR) - 1u;
  uint32_t full_kc = 0u, full_kr = 0u;
  for (int i = 0; i < H; ++i) {
    full_kc |= cmask << (5 * i);
    full_kr |= rmask << (5 * i);
  }
  for (int p = 0; p < P; ++p) {
    uint32_t hw = 0;
    for (int i = 0; i < H; ++i) hw |= (uint32_t)sc[p * H + i] << (5 * i);
    GP(PLH(p)) = hw | ((uint32_t)H << 25);
    GP(PLKCP(p)) = full_kc;
    GP(PLKRP(p)) = full_kr;
    GP(PLKH(p)) = 0u;
  }
  GP(PL_DECK_LO) = (uint32_t)deck;
  GP(PL_DECK_HI) = (uint32_t)(deck >> 32);
  GP(PL_DISC_LO) = 0u;
  GP(PL_DISC_HI) = 0u;
  // the board of a reset after its deal: full tokens, no fireworks, P turns to play, seat 0 on turn, seat 1 % P next
  GP(PL_BOARD) = ((uint32_t)ep.max_info << 15) | ((uint32_t)ep.max_life << 19) | ((uint32_t)P << 21) | (1u << 24) | ((uint32_t)(1 % P) << 27);
  // step 0, deck size, not terminated, started; last score [16..21] and the look-ahead count [22..23] kept
  GP(PL_MISC) = (misc & ((63u << 16) | (3u << 22))) | ((uint32_t)(ep.deck_max - P * H) << 8) | (1u << 15);
  GP(PL_LASTMV) = 0u;
  sel[g] = g;
}

// ---- playout: policy -> step until the games end, no restart, no observation rows --------------------------------------------------
// One wave per 64 games; the planes stay in LDS and the generator context in registers for the whole launch.  Per iteration and live
// game: the policy writes the actions of this iteration (a_out / g_out, all P seats of the lane's game), then the step of MODE 1 runs
// on the actions just written.  key (or the game index) is the "game" field of the policy hash.  A lane whose game is finished does
// nothing; the wave leaves the loop when none of its games is live, so a launch does at most n_iter iterations and never looks at
// another workgroup.  Afterwards: look-ahead topped up as a step leaves it, planes written back, `terminal` and the legal masks the
// next policy call reads made current.
//
// policy (by value, its call inlined): act<TH>(ep, s_st, lane, g, P, H, ru, pkey, counter) writes ep.a_out / ep.g_out [g, 0..P) for
// the lane's live game from the planes in s_st; counter is the game's policy counter before this iteration.
//
// The two kernels' code is not what it was when each spelled this body out, and neither the helpers, the accessors nor the policy
// object are why: the old kernel text moved verbatim into a force-inlined __device__ function gives the same new code (the kernel's
// parameter struct then reaches the body through a reference, as it always did in env_body).  tools/isa_compare.py shows the sizes.
template <int TP, int TH, bool V, class Policy>
__device__ __forceinline__ void playout_body(const EnvParams& ep, const int64_t* __restrict__ key, const Policy policy) {
  extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
  uint32_t* s_st = smem;
  const int lane = threadIdx.x;
  const int g = blockIdx.x * kWave + lane;   // < Gpad
  const bool valid = g < ep.G;
  const int P = TP ? TP : ep.P, H = TH ? TH : ep.H;
  const auto ru = RulesOf<V>::make(ep);
  stage_planes(ep, s_st, lane, g);
  const uint32_t misc0 = ST(PL_MISC);
  const bool live0 = valid && misc_live(misc0);
  if (__ballot(live0) == 0ull) return;
  const uint64_t pkey = valid ? (key ? (uint64_t)key[g] : (uint64_t)g) : 0ull;
  Rng rng = rng_open(ep, s_st, lane, g, misc0);
#pragma clang loop unroll(disable)
  for (int it = 0; it < ep.n_iter; ++it) {
    const bool live = live0 && !misc_term(ST(PL_MISC));
    if (__ballot(live) == 0ull) break;
    if (live) {
      const uint32_t counter = ep.act_count[g];
      ep.act_count[g] = counter + 1u;
      policy.template act<TH>(ep, s_st, lane, g, P, H, ru, pkey, counter);
    }
    uint32_t greedy_rec = 0;
    float reward = 0.f;
    bool term = false;
    env_logic<1, TP, TH, V>(ep, ep.a_out, ep.g_out, s_st, nullptr, nullptr, lane, g, live, false, rng, greedy_rec, reward, term);
  }
  if (live0) {
    Refill rf;
    refill_issue(rf, rng, true);
    refill_finish(rf, rng);
    rng_close(rng, s_st, lane);
    for (int p = 0; p < P; ++p)
      ep.legal_bits[(size_t)g * P + p] =
          legal_mask_of<TH>(P, H, ep.A, s_st, lane, p, ep.shuffle_color ? (ST(PLPERM(p)) & 0x7fffu) : kIdentityPerm, ru);
    for (int pl = 0; pl < ep.npl; ++pl) ep.planes[(size_t)pl * ep.Gpad + g] = ST(pl);
    ep.terminal[g] = (uint8_t)misc_term(ST(PL_MISC));
  }
}

// the policy of policy_kernel on the legal masks of the state itself (the masks build_rows would have stored)
struct RandomLegalPolicy {
  template <int TH, class Ru>
  __device__ __forceinline__ void act(const EnvParams& ep, const uint32_t* s_st, int lane, int g, int P, int H, const Ru& ru, uint64_t pkey,
                                      uint32_t counter) const {
    for (int p = 0; p < P; ++p) {
      const uint64_t mask = legal_mask_of<TH>(P, H, ep.A, s_st, lane, p, ep.shuffle_color ? (ST(PLPERM(p)) & 0x7fffu) : kIdentityPerm, ru);
      ep.a_out[(size_t)g * P + p] = policy_pick(ep.policy_seed, pkey, (uint64_t)counter, p, 0, mask);
      if (ep.g_out) ep.g_out[(size_t)g * P + p] = policy_pick(ep.policy_seed, pkey, (uint64_t)counter, p, 1, mask);
    }
  }
};

template <int TP, int TH, bool V>
__global__ __launch_bounds__(kWave) void env_playout_kernel(EnvParams ep, const int64_t* __restrict__ key) {
  playout_body<TP, TH, V>(ep, key, RandomLegalPolicy{});
}

typedef void (*EnvObserveFn)(EnvParams, ObserveArgs);
typedef void (*EnvPlayoutFn)(EnvParams, const int64_t*);

EnvObserveFn pick_observe_kernel(const EnvParams& ep) {
  if (ep.variant) return env_observe_kernel<0, 0, true>;
  if (ep.P == 2 && ep.H == 5) return env_observe_kernel<2, 5, false>;
  return env_observe_kernel<0, 0, false>;
}
EnvPlayoutFn pick_playout_kernel(const EnvParams& ep) {
  if (ep.variant) return env_playout_kernel<0, 0, true>;
  if (ep.P == 2 && ep.H == 5) return env_playout_kernel<2, 5, false>;
  return env_playout_kernel<0, 0, false>;
}

int launch_observe(hsad_env* e, const ObserveArgs& oa, hipStream_t stream) {
  const EnvParams& ep = e->ep;
  const void* fn = reinterpret_cast<const void*>(pick_observe_kernel(ep));
  // per launch: envs of different shapes share one kernel and the attribute belongs to the kernel
  HIP_TRY(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)e->lds_bytes));
  hipLaunchKernelGGL(pick_observe_kernel(ep), dim3((ep.G + ep.gpw - 1) / ep.gpw), dim3(ep.nthreads), e->lds_bytes, stream, ep, oa);
  HIP_TRY(hipGetLastError());
  return HSAD_OK;
}

// where the SAD section of `src`'s current rows can be read from; false when it has no observation output that holds it
bool sad_source(const hsad_env* src, ObserveArgs* oa) {
  oa->sad_bits = nullptr;
  oa->sad_f32 = nullptr;
  oa->sad_words = nullptr;
  oa->sad_pw64 = 0;
  if (src->ep.priv_bits) {
    oa->sad_bits = src->ep.priv_bits;
    oa->sad_pw64 = src->ep.pw64;
    return true;
  }
  if (src->bound && src->ep.obs_f32 && src->ep.priv_s) {
    oa->sad_f32 = src->ep.priv_s;
    return true;
  }
  return false;
}

}  // namespace

extern "C" {

int hsad_env_fork(hsad_env* dst, hsad_env* src, const int32_t* src_index, const int32_t* seeds, void* stream) {
  if (!dst || !src || !src_index) return set_error(HSAD_ERR_INVALID, "null argument");
  if (dst == src) return set_error(HSAD_ERR_INVALID, "hsad_env_fork: dst and src are the same env");
  const EnvParams &d = dst->ep, &s = src->ep;
  if (d.P != s.P || d.H != s.H) return set_error(HSAD_ERR_INVALID, "hsad_env_fork: players / hand size differ");
  if (d.nC != s.nC || d.nR != s.nR || d.max_info != s.max_info || d.max_life != s.max_life)
    return set_error(HSAD_ERR_INVALID, "hsad_env_fork: the game's rules differ");
  if (d.sad != s.sad || d.shuffle_color != s.shuffle_color || d.kmode != s.kmode || d.bomb != s.bomb || d.max_len != s.max_len)
    return set_error(HSAD_ERR_INVALID, "hsad_env_fork: sad / shuffle_color / knowledge_mode / bomb / max_len differ");
  if (dst->device != src->device) return set_error(HSAD_ERR_INVALID, "hsad_env_fork: the envs live on different devices");
  if (d.track_dh && !s.track_dh) return set_error(HSAD_ERR_INVALID, "hsad_env_fork: dst tracks the deck history and src does not");
  if (!dst->bound) return set_error(HSAD_ERR_STATE, "hsad_env_bind_outputs must be called first (dst)");
  ObserveArgs oa;
  oa.sel = src_index;
  oa.sel_limit = s.G;
  if (!sad_source(src, &oa) && d.sad)
    return set_error(HSAD_ERR_INVALID, "hsad_env_fork: sad = 1 needs src's observation rows (float32 or bit words) to copy the greedy-action section from");
  hipLaunchKernelGGL(env_fork_kernel, dim3((d.G + 3) / 4), dim3(4 * kWave), 0, (hipStream_t)stream, d, s, src_index, seeds,
                     (d.track_dh && s.track_dh) ? 1 : 0);
  HIP_TRY(hipGetLastError());
  return launch_observe(dst, oa, (hipStream_t)stream);
}

int hsad_env_determinize(hsad_env* e, const int32_t* viewer, const int64_t* key, uint64_t seed, int32_t* tries_out, void* stream) {
  if (!e || !viewer || !key) return set_error(HSAD_ERR_INVALID, "null argument");
  if (!e->bound) return set_error(HSAD_ERR_STATE, "hsad_env_bind_outputs must be called first");
  ObserveArgs oa;
  if (!sad_source(e, &oa) && e->ep.sad)
    return set_error(HSAD_ERR_INVALID, "hsad_env_determinize: sad = 1 needs the env's own observation rows (float32 or bit words)");
  if (!e->d_sel) {
    HIP_TRY(hipSetDevice(e->device));
    HIP_TRY(hipMalloc((void**)&e->d_sel, sizeof(int32_t) * (size_t)e->ep.Gpad));
  }
  oa.sel = e->d_sel;
  oa.sel_limit = e->ep.G;
  hipLaunchKernelGGL(env_determinize_kernel, dim3((e->ep.G + 255) / 256), dim3(256), 0, (hipStream_t)stream, e->ep, viewer, key, seed,
                     tries_out, e->d_sel);
  HIP_TRY(hipGetLastError());
  return launch_observe(e, oa, (hipStream_t)stream);
}

int hsad_env_rewind_scripted(hsad_env* e, const uint8_t* script, const int32_t* count, void* stream) {
  if (!e || !script || !count) return set_error(HSAD_ERR_INVALID, "null argument");
  if (!e->bound) return set_error(HSAD_ERR_STATE, "hsad_env_bind_outputs must be called first");
  const int Gpad = e->ep.Gpad;
  HIP_TRY(hipSetDevice(e->device));
  if (!e->d_sel) HIP_TRY(hipMalloc((void**)&e->d_sel, sizeof(int32_t) * (size_t)Gpad));
  if (!e->script.cards) HIP_TRY(hipMalloc((void**)&e->script.cards, (size_t)Gpad * 52));
  if (!e->script.count) HIP_TRY(hipMalloc((void**)&e->script.count, sizeof(int32_t) * (size_t)Gpad));
  if (!e->scripted) {   // the first script since creation / reset: no game has one yet
    HIP_TRY(hipMemsetAsync(e->script.cards, 0, (size_t)Gpad * 52, (hipStream_t)stream));
    HIP_TRY(hipMemsetAsync(e->script.count, 0, sizeof(int32_t) * (size_t)Gpad, (hipStream_t)stream));
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(pick_scripted_step_kernel(e->ep.P, e->ep.H, e->ep.variant != 0)),
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)e->lds_bytes));
    e->scripted = true;
  }
  hipLaunchKernelGGL(env_rewind_kernel, dim3((e->ep.G + 255) / 256), dim3(256), 0, (hipStream_t)stream, e->ep, e->script, script, count, e->d_sel);
  HIP_TRY(hipGetLastError());
  ObserveArgs oa;
  oa.sel = e->d_sel;
  oa.sel_limit = e->ep.G;
  oa.sad_bits = nullptr;   // no move has been made: the SAD section of a rewound game is all-zero
  oa.sad_f32 = nullptr;
  oa.sad_words = nullptr;
  oa.sad_pw64 = 0;
  return launch_observe(e, oa, (hipStream_t)stream);
}

int hsad_env_sad_section(hsad_env* e, int64_t* out, void* stream) {
  if (!e || !out) return set_error(HSAD_ERR_INVALID, "null argument");
  if (!e->bound) return set_error(HSAD_ERR_STATE, "hsad_env_bind_outputs must be called first");
  ObserveArgs oa;
  oa.sel = nullptr;
  oa.sel_limit = 0;
  if (!sad_source(e, &oa) && e->ep.sad)
    return set_error(HSAD_ERR_INVALID, "hsad_env_sad_section: sad = 1 needs the env's own observation rows (float32 or bit words)");
  const int n = e->ep.G * e->ep.P;
  hipLaunchKernelGGL(env_sad_section_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, e->ep, oa,
                     reinterpret_cast<unsigned long long*>(out));
  HIP_TRY(hipGetLastError());
  return HSAD_OK;
}

int hsad_env_observe_sad(hsad_env* e, const int32_t* src_index, int G_src, const int64_t* sad, void* stream) {
  if (!e || !src_index || !sad) return set_error(HSAD_ERR_INVALID, "null argument");
  if (!e->bound) return set_error(HSAD_ERR_STATE, "hsad_env_bind_outputs must be called first");
  if (G_src < 1) return set_error(HSAD_ERR_INVALID, "hsad_env_observe_sad: G_src must be >= 1");
  if (!e->ep.sad) return HSAD_OK;   // the rows have no such section
  ObserveArgs oa;
  oa.sel = src_index;
  oa.sel_limit = G_src;
  oa.sad_bits = nullptr;
  oa.sad_f32 = nullptr;
  oa.sad_words = reinterpret_cast<const unsigned long long*>(sad);
  oa.sad_pw64 = 0;
  return launch_observe(e, oa, (hipStream_t)stream);
}

// shared with csrc/hsad_search.hip (not part of the public header): the hand planes hsad_search_world_script reads
int hsad_internal_env_hands(const hsad_env* e, const uint32_t** hand0, int* G, int* Gpad, int* P, int* H) {
  if (!e) return set_error(HSAD_ERR_INVALID, "null env");
  *hand0 = e->ep.planes + (size_t)PL_FIXED * e->ep.Gpad;   // plane PLH(p) = hand0 + p * Gpad
  *G = e->ep.G;
  *Gpad = e->ep.Gpad;
  *P = e->ep.P;
  *H = e->ep.H;
  return HSAD_OK;
}

// shared with csrc/hsad_search.hip: the legal-move masks [G, P] (bit uid) of the rows the env wrote last
int hsad_internal_env_legal_bits(const hsad_env* e, const unsigned long long** legal_bits) {
  if (!e) return set_error(HSAD_ERR_INVALID, "null env");
  *legal_bits = e->ep.legal_bits;
  return HSAD_OK;
}

int hsad_env_playout_random_keyed(hsad_env* e, int max_iter, uint64_t policy_seed, const int64_t* key, int64_t* a, int64_t* greedy_a,
                                  void* stream) {
  if (!e) return set_error(HSAD_ERR_INVALID, "null env");
  if (!e->bound) return set_error(HSAD_ERR_STATE, "hsad_env_bind_outputs must be called first");
  if (!a) return set_error(HSAD_ERR_INVALID, "action tensor is null");
  if (e->ep.sad && !greedy_a) return set_error(HSAD_ERR_INVALID, "sad=1 requires greedy_a");
  if (max_iter < 0) return set_error(HSAD_ERR_INVALID, "max_iter must be >= 0");
  if (e->scripted)
    return set_error(HSAD_ERR_STATE, "hsad_env_playout_random: the env holds a deal script (only hsad_env_step deals from it; hsad_env_reset clears it)");
  if (max_iter == 0) return HSAD_OK;
  EnvParams ep = e->ep;
  ep.policy_seed = policy_seed;
  ep.n_iter = max_iter;
  ep.a_out = a;
  ep.g_out = greedy_a;
  ep.dbg = nullptr;
  hipLaunchKernelGGL(pick_playout_kernel(ep), dim3(ep.Gpad / kWave), dim3(kWave), sizeof(uint32_t) * (size_t)ep.npl * kWave,
                     (hipStream_t)stream, ep, key);
  HIP_TRY(hipGetLastError());
  return HSAD_OK;
}

int hsad_env_playout_random(hsad_env* e, int max_iter, uint64_t policy_seed, int64_t* a, int64_t* greedy_a, void* stream) {
  return hsad_env_playout_random_keyed(e, max_iter, policy_seed, nullptr, a, greedy_a, stream);
}

}  // extern "C"
