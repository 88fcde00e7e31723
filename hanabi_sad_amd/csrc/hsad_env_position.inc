// hsad_env_position.inc — positions in and out of an env: import of the canonical record hsad_env_export_state writes, and a
// complete per-game snapshot with its restore.  Textually part of hsad_env.hip (included at its end, after hsad_env_search.inc,
// whose observe pass rewrites the rows of the games these calls change).
//
// Nothing here is reached by reset / step / rollout / fork: the three kernels are separate launches, EnvParams is what it was, and
// every existing kernel is compiled from unchanged code.  Plain loads and vector stores only; the one atomic is log_error's.

#include "hsad_position.h"

namespace {

__host__ __device__ inline PosRules pos_rules_of(const EnvParams& ep) {
  return PosRules{ep.P, ep.H, ep.nC, ep.nR, ep.max_info, ep.max_life, ep.max_len, ep.shuffle_color, ep.deck_full};
}

// std::mt19937(seed)'s 624 words: init_game's and env_fork_kernel's seeding
__device__ __forceinline__ void seed_generator(uint32_t* mt, uint32_t x) {
  mt[0] = x;
  for (int i = 1; i < kMtN; ++i) {
    x = 1812433253u * (x ^ (x >> 30)) + (uint32_t)i;
    mt[i] = x;
  }
}

// ---- import: the canonical record -> the game's planes ----------------------------------------------------------------------------
// One thread per game, the shape of env_rewind_kernel.  The record is decoded into local plane words and checked there; a game is
// written only after its record passed.  sel[g] = g for the imported games (the observe pass that follows rewrites their rows).
__global__ void env_import_kernel(EnvParams ep, DealScript own, const int32_t* __restrict__ states, int words,
                                  const uint8_t* __restrict__ take, const int32_t* __restrict__ seeds, const float* __restrict__ eps,
                                  int32_t* __restrict__ status, int32_t* __restrict__ sel) {
  const int g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= ep.G) return;
  sel[g] = -1;
  if (!take[g]) {
    if (status) status[g] = -1;
    return;
  }
  const int P = ep.P;
  const PosRules r = pos_rules_of(ep);
  uint32_t w[POS_MAX_PLANES];
  uint32_t flags = pos_decode_record(states + (size_t)g * words, r, w);
  const uint32_t misc0 = GP(PL_MISC);
  const bool started = misc_started(misc0);
  if (!(flags & (HSAD_POS_FIELD | HSAD_POS_HANDS))) flags |= position_valid(w, r);
  if (!seeds && !started) flags |= HSAD_POS_NO_GENERATOR;
  if (status) status[g] = (int32_t)flags;
  if (flags) {
    log_error(ep, g, 6);
    return;
  }
  for (int pl = 0; pl <= PL_LASTMV; ++pl)
    if (pl != PL_MISC) GP(pl) = w[pl];
  // the look-ahead count stays with the generator that is kept
  GP(PL_MISC) = w[PL_MISC] | (seeds ? 0u : (misc0 & (3u << 22)));
  for (int p = 0; p < P; ++p) {
    GP(PLH(p)) = w[PLH(p)];
    GP(PLKCP(p)) = w[PLKCP(p)];
    GP(PLKRP(p)) = w[PLKRP(p)];
    GP(PLKH(p)) = w[PLKH(p)];
    GP(PLPERM(p)) = w[PLPERM(p)];
    if (eps)
      GP(PLEPS(p)) = __float_as_uint(eps[(size_t)g * P + p]);
    else if (!started)
      GP(PLEPS(p)) = 0u;
  }
  if (seeds) {
    GP(PL_DRAWS) = 0u;
    GP(PL_LA0) = 0u;
    GP(PL_LA1) = 0u;
    seed_generator(ep.mt + (size_t)g * kMtN, (uint32_t)seeds[g]);
  }
  // the cards of an imported position have no deal order
  if (ep.track_dh)
    for (int i = 0; i < 52; ++i) ep.deck_hist[(size_t)g * 52 + i] = (uint8_t)0;
  if (own.cards) {
    for (int i = 0; i < 52; ++i) own.cards[(size_t)g * 52 + i] = (uint8_t)0;
    own.count[g] = 0;
  }
  sel[g] = g;
}

// ---- snapshot: everything that decides what a game does and shows next, as one fixed-size record ------------------------------------
// Record of 32-bit words (offsets in words; hsad.h documents them): planes [0, npl) | policy counter | 624 generator words |
// deck-history row, 13 words (if tracked) | deal-script row, 13 words, and count (if the env holds a script) | SAD section, 2 words
// per seat.  A function of (P, H, track_deck_history, script held) only.
struct SnapLayout {
  int npl, off_cnt, off_mt, off_dh, off_sc, off_sad, words, has_dh, has_sc;
};
constexpr int kSnapMaxWords = POS_MAX_PLANES + 1 + kMtN + 13 + 14 + 2 * POS_MAX_PLAYERS;

SnapLayout snap_layout(const EnvParams& ep, bool script) {
  SnapLayout l;
  l.npl = ep.npl;
  l.off_cnt = l.npl;
  l.off_mt = l.off_cnt + 1;
  l.has_dh = ep.track_dh ? 1 : 0;
  l.has_sc = script ? 1 : 0;
  l.off_dh = l.off_mt + kMtN;
  l.off_sc = l.off_dh + (l.has_dh ? 13 : 0);
  l.off_sad = l.off_sc + (l.has_sc ? 14 : 0);
  l.words = l.off_sad + 2 * ep.P;
  return l;
}

// One wave per game, as in env_fork_kernel: the lanes walk the record's words, so its stores are coalesced.
__global__ void env_snapshot_kernel(EnvParams ep, DealScript own, ObserveArgs oa, SnapLayout l, uint32_t* __restrict__ out) {
  const int lane = threadIdx.x & (kWave - 1);
  const int j = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (j >= ep.G) return;
  uint32_t* rec = out + (size_t)j * l.words;
  for (int pl = lane; pl < l.npl; pl += kWave) rec[pl] = ep.planes[(size_t)pl * ep.Gpad + j];
  if (lane == 0) rec[l.off_cnt] = ep.act_count[j];
  const uint32_t* mt = ep.mt + (size_t)j * kMtN;
  for (int k = lane; k < kMtN; k += kWave) rec[l.off_mt + k] = mt[k];
  if (l.has_dh && lane < 13) rec[l.off_dh + lane] = reinterpret_cast<const uint32_t*>(ep.deck_hist + (size_t)j * 52)[lane];
  if (l.has_sc) {
    if (lane < 13) rec[l.off_sc + lane] = reinterpret_cast<const uint32_t*>(own.cards + (size_t)j * 52)[lane];
    if (lane == 13) rec[l.off_sc + 13] = (uint32_t)own.count[j];
  }
  if (lane < ep.P) {
    const uint64_t v = ep.sad ? sad_section_of(ep, oa, (size_t)j * ep.P + lane) : 0ull;
    rec[l.off_sad + 2 * lane] = (uint32_t)v;
    rec[l.off_sad + 2 * lane + 1] = (uint32_t)(v >> 32);
  }
}

// What a record must satisfy beyond position_valid, on the record's words in LDS (one lane).
__device__ uint32_t snapshot_record_valid(const EnvParams& ep, const SnapLayout& l, const uint32_t* rec) {
  const uint32_t misc = rec[PL_MISC];
  uint32_t f = 0;
  if (misc_la_n(misc) > 2) f |= HSAD_POS_LOOKAHEAD;
  // the history and the script are written with the game whatever its state: their ranges hold for every record
  if (l.has_dh) {
    const uint8_t* dh = reinterpret_cast<const uint8_t*>(rec + l.off_dh);
    for (int i = 0; i < 52; ++i)
      if (dh[i] >= 25) f |= HSAD_POS_HISTORY;
  }
  const uint8_t* sc = reinterpret_cast<const uint8_t*>(rec + l.off_sc);   // (read only with has_sc)
  const int n = l.has_sc ? (int)rec[l.off_sc + 13] : 0;
  bool script_ok = false;
  if (l.has_sc) {
    if (n < 0 || n > ep.deck_max || (n > 0 && n < ep.P * ep.H)) {
      f |= HSAD_POS_HISTORY;
    } else {
      script_ok = true;
      for (int i = 0; i < n; ++i) script_ok &= sc[i] < 25;
      if (!script_ok) f |= HSAD_POS_HISTORY;
    }
  }
  if (!misc_started(misc)) return f;   // never started: its planes are restored as they are (a reset overwrites every one it reads)
  const PosRules r = pos_rules_of(ep);
  const uint32_t pv = position_valid(rec, r);
  f |= pv & ~(uint32_t)HSAD_POS_TERMINAL;
  const bool term = misc_term(misc);
  if (term != ((pv & HSAD_POS_TERMINAL) != 0u)) f |= HSAD_POS_RECORD;   // the terminated bit is what the position says
  if (script_ok && !term && !(f & HSAD_POS_CONSERVATION)) {
    // the deals still to come from the script, on the deck the record holds
    uint64_t pool = (uint64_t)rec[PL_DECK_LO] | ((uint64_t)rec[PL_DECK_HI] << 32);
    for (int i = ep.deck_max - misc_deck_size(misc); i < n; ++i) {
      const int t = sc[i];
      if (cnt2(pool, t) == 0u) {
        f |= HSAD_POS_SCRIPT;
        break;
      }
      pool -= (uint64_t)1 << (2 * t);
    }
  }
  return f;
}

// ---- restore: dst game j becomes record src_index[j] ------------------------------------------------------------------------------
// One wave (= one workgroup) per destination game.  The record is read once into LDS, coalesced; lane 0 checks it; only then do
// the lanes write the game.  dst_script: the env holds script buffers (a record without a script then clears the game's script).
__global__ __launch_bounds__(kWave) void env_restore_kernel(EnvParams ep, DealScript own, SnapLayout l, const uint32_t* __restrict__ in,
                                                            int G_src, const int32_t* __restrict__ src_index,
                                                            unsigned long long* __restrict__ sad_words, int32_t* __restrict__ status,
                                                            int32_t* __restrict__ sel) {
  __shared__ uint32_t s_rec[kSnapMaxWords];
  __shared__ uint32_t s_flags;
  const int lane = threadIdx.x;
  const int j = blockIdx.x;   // < G
  const int si = src_index ? src_index[j] : j;
  if (si < 0 || si >= G_src) {   // uniform over the workgroup
    if (lane == 0) {
      sel[j] = -1;
      if (status) status[j] = -1;
      if (si != -1) log_error(ep, j, 4);
    }
    return;
  }
  const uint32_t* src = in + (size_t)si * l.words;
  for (int k = lane; k < l.words; k += kWave) s_rec[k] = src[k];
  __syncthreads();
  if (lane == 0) s_flags = snapshot_record_valid(ep, l, s_rec);
  __syncthreads();
  const uint32_t flags = s_flags;
  if (flags) {
    if (lane == 0) {
      sel[j] = -1;
      if (status) status[j] = (int32_t)flags;
      log_error(ep, j, 6);
    }
    return;
  }
  for (int pl = lane; pl < l.npl; pl += kWave) ep.planes[(size_t)pl * ep.Gpad + j] = s_rec[pl];
  uint32_t* mt = ep.mt + (size_t)j * kMtN;
  for (int k = lane; k < kMtN; k += kWave) mt[k] = s_rec[l.off_mt + k];
  if (l.has_dh && lane < 13) reinterpret_cast<uint32_t*>(ep.deck_hist + (size_t)j * 52)[lane] = s_rec[l.off_dh + lane];
  if (own.cards) {
    if (lane < 13) reinterpret_cast<uint32_t*>(own.cards + (size_t)j * 52)[lane] = l.has_sc ? s_rec[l.off_sc + lane] : 0u;
    if (lane == 13) own.count[j] = l.has_sc ? (int32_t)s_rec[l.off_sc + 13] : 0;
  }
  if (lane < ep.P)
    sad_words[(size_t)j * ep.P + lane] = (unsigned long long)s_rec[l.off_sad + 2 * lane] | ((unsigned long long)s_rec[l.off_sad + 2 * lane + 1] << 32);
  if (lane == 0) {
    ep.act_count[j] = s_rec[l.off_cnt];
    sel[j] = j;
    if (status) status[j] = 0;
  }
}

int ensure_sel(hsad_env* e) {
  if (!e->d_sel) {
    HIP_TRY(hipSetDevice(e->device));
    HIP_TRY(hipMalloc((void**)&e->d_sel, sizeof(int32_t) * (size_t)e->ep.Gpad));
  }
  return HSAD_OK;
}

// the env takes up a script (what the first hsad_env_rewind_scripted does): buffers, all counts 0, the scripted step kernel
int ensure_script(hsad_env* e, hipStream_t stream) {
  if (e->scripted) return HSAD_OK;
  const int Gpad = e->ep.Gpad;
  HIP_TRY(hipSetDevice(e->device));
  if (!e->script.cards) HIP_TRY(hipMalloc((void**)&e->script.cards, (size_t)Gpad * 52));
  if (!e->script.count) HIP_TRY(hipMalloc((void**)&e->script.count, sizeof(int32_t) * (size_t)Gpad));
  HIP_TRY(hipMemsetAsync(e->script.cards, 0, (size_t)Gpad * 52, stream));
  HIP_TRY(hipMemsetAsync(e->script.count, 0, sizeof(int32_t) * (size_t)Gpad, stream));
  HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(pick_scripted_step_kernel(e->ep.P, e->ep.H, e->ep.variant != 0)),
                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)e->lds_bytes));
  e->scripted = true;
  return HSAD_OK;
}

}  // namespace

extern "C" {

int hsad_env_import_state(hsad_env* e, const int32_t* states, const uint8_t* take, const int32_t* seeds, const float* eps,
                          int32_t* status, void* stream) {
  if (!e || !states || !take) return set_error(HSAD_ERR_INVALID, "null argument");
  if (!e->bound) return set_error(HSAD_ERR_STATE, "hsad_env_bind_outputs must be called first");
  if (e->ep.P > POS_MAX_PLAYERS || e->ep.H > 5) return set_error(HSAD_ERR_INVALID, "hsad_env_import_state: more than 5 players or 5 cards a hand");
  int rc = ensure_sel(e);
  if (rc != HSAD_OK) return rc;
  // while the env holds a script, the imported games leave it: their script rows and counts are cleared
  hipLaunchKernelGGL(env_import_kernel, dim3((e->ep.G + 255) / 256), dim3(256), 0, (hipStream_t)stream, e->ep,
                     e->scripted ? e->script : DealScript{nullptr, nullptr}, states, hsad_env_state_words(e), take, seeds, eps, status, e->d_sel);
  HIP_TRY(hipGetLastError());
  ObserveArgs oa;
  oa.sel = e->d_sel;
  oa.sel_limit = e->ep.G;
  oa.sad_bits = nullptr;   // the record holds no greedy action: the SAD section of an imported game is all-zero
  oa.sad_f32 = nullptr;
  oa.sad_words = nullptr;
  oa.sad_pw64 = 0;
  return launch_observe(e, oa, (hipStream_t)stream);
}

int64_t hsad_env_snapshot_record_bytes(const hsad_env* e) {
  return e ? (int64_t)sizeof(uint32_t) * snap_layout(e->ep, e->scripted).words : 0;
}

int hsad_env_snapshot(hsad_env* e, void* out, void* stream) {
  if (!e || !out) return set_error(HSAD_ERR_INVALID, "null argument");
  if (!e->bound) return set_error(HSAD_ERR_STATE, "hsad_env_bind_outputs must be called first");
  if ((uintptr_t)out & 3u) return set_error(HSAD_ERR_INVALID, "hsad_env_snapshot: out must be 4-byte aligned");
  if (e->ep.P > POS_MAX_PLAYERS) return set_error(HSAD_ERR_INVALID, "hsad_env_snapshot: more than 5 players");
  ObserveArgs oa;
  oa.sel = nullptr;
  oa.sel_limit = 0;
  if (!sad_source(e, &oa) && e->ep.sad)
    return set_error(HSAD_ERR_INVALID, "hsad_env_snapshot: sad = 1 needs the env's own observation rows (float32 or bit words)");
  hipLaunchKernelGGL(env_snapshot_kernel, dim3((e->ep.G + 3) / 4), dim3(4 * kWave), 0, (hipStream_t)stream, e->ep,
                     e->scripted ? e->script : DealScript{nullptr, nullptr}, oa, snap_layout(e->ep, e->scripted), static_cast<uint32_t*>(out));
  HIP_TRY(hipGetLastError());
  return HSAD_OK;
}

int hsad_env_restore(hsad_env* e, const void* in, int64_t record_bytes, int G_src, const int32_t* src_index, int32_t* status, void* stream) {
  if (!e || !in) return set_error(HSAD_ERR_INVALID, "null argument");
  if (!e->bound) return set_error(HSAD_ERR_STATE, "hsad_env_bind_outputs must be called first");
  if ((uintptr_t)in & 3u) return set_error(HSAD_ERR_INVALID, "hsad_env_restore: in must be 4-byte aligned");
  if (e->ep.P > POS_MAX_PLAYERS) return set_error(HSAD_ERR_INVALID, "hsad_env_restore: more than 5 players");
  if (G_src < 1) return set_error(HSAD_ERR_INVALID, "hsad_env_restore: G_src must be >= 1");
  if (!src_index && G_src != e->ep.G) return set_error(HSAD_ERR_INVALID, "hsad_env_restore: src_index == NULL needs G_src == G");
  const SnapLayout plain = snap_layout(e->ep, false), scripted = snap_layout(e->ep, true);
  const bool with_script = record_bytes == (int64_t)sizeof(uint32_t) * scripted.words;
  if (!with_script && record_bytes != (int64_t)sizeof(uint32_t) * plain.words)
    return set_error(HSAD_ERR_INVALID, "hsad_env_restore: records of %lld bytes, this env's are %lld (%lld with a deal script)",
                     (long long)record_bytes, (long long)(sizeof(uint32_t) * plain.words), (long long)(sizeof(uint32_t) * scripted.words));
  int rc = ensure_sel(e);
  if (rc != HSAD_OK) return rc;
  if (with_script && (rc = ensure_script(e, (hipStream_t)stream)) != HSAD_OK) return rc;
  if (!e->d_sad) {
    HIP_TRY(hipSetDevice(e->device));
    HIP_TRY(hipMalloc((void**)&e->d_sad, sizeof(unsigned long long) * (size_t)e->ep.Gpad * e->ep.P));
  }
  hipLaunchKernelGGL(env_restore_kernel, dim3(e->ep.G), dim3(kWave), 0, (hipStream_t)stream, e->ep,
                     e->scripted ? e->script : DealScript{nullptr, nullptr}, with_script ? scripted : plain, static_cast<const uint32_t*>(in), G_src,
                     src_index, e->d_sad, status, e->d_sel);
  HIP_TRY(hipGetLastError());
  ObserveArgs oa;
  oa.sel = e->d_sel;
  oa.sel_limit = e->ep.G;
  oa.sad_bits = nullptr;
  oa.sad_f32 = nullptr;
  oa.sad_words = e->d_sad;   // row sel[g] * P + p = g * P + p: the recorded section of the game itself
  oa.sad_pw64 = 0;
  return launch_observe(e, oa, (hipStream_t)stream);
}

}  // extern "C"
