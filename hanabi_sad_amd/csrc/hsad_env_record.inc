// hsad_env_record.inc — replay of game records (include/hsad.h: hsad_env_playout_logged): game j becomes a record played from its
// first deal up to a chosen move, in one launch.  Textually part of hsad_env.hip (included at its end: the kernels below use its
// state planes, its game logic, the rewind and observe kernels of hsad_env_search.inc as they are).  Record layout:
// hsad_game_record.h.
//
// Nothing here is reached by reset / step / rollout or by the existing playouts: the two kernels are separate launches, EnvParams is
// what it was, and env_playout_kernel / env_playout_rule_kernel keep refusing an env that holds a deal script.  The replay is the
// playout of hsad_env_search.inc with two differences that playout_body's loop has no room for: the step is the SCRIPTED
// instantiation of the MODE-1 logic (env_logic over ScriptedParams: next_card reads the record's deck), and a lane stops on its own
// (at stop[j], or at a logged move that is illegal) instead of at the end of its game.

#include "hsad_game_record.h"

namespace {

// record src_index[g] -> the game's script row and count for env_rewind_kernel; status: SKIPPED / BAD_INDEX now, REFUSED until the
// playout kernel overwrites it for the games the rewind took
__global__ void env_logged_prep_kernel(EnvParams ep, const uint8_t* __restrict__ records, int n_rec, int rec_bytes,
                                       const int32_t* __restrict__ src_index, uint8_t* __restrict__ script, int32_t* __restrict__ count,
                                       int32_t* __restrict__ status) {
  const int g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= ep.G) return;
  count[g] = 0;
  const int si = src_index[g];
  if (si == -1) {
    status[g] = HSAD_GR_STATUS_SKIPPED;
    return;
  }
  if (si < 0 || si >= n_rec) {
    log_error(ep, g, 4);
    status[g] = HSAD_GR_STATUS_BAD_INDEX;
    return;
  }
  const uint8_t* rec = records + (size_t)si * rec_bytes;
  const int n = rec[GR_OFF_NDEALT];
  for (int i = 0; i < 52; ++i) script[(size_t)g * 52 + i] = rec[GR_OFF_DECK + i];
  // a record of a game that was never dealt has nothing to rewind to: an impossible count, which the rewind logs as code 5
  count[g] = n > 0 ? n : 1;
  status[g] = HSAD_GR_STATUS_REFUSED;
}

// One wave per 64 games, the shape of playout_body: planes in LDS, generator context in registers; behind the planes the move and
// greedy planes of the wave's records, time-major [2 L][64] bytes, so that the lanes of an iteration read neighbouring bytes.
// sel[g] == g marks the games env_rewind_kernel has just rewound; every other lane is left alone.
template <int TP, int TH, bool V>
__global__ __launch_bounds__(kWave) void env_playout_logged_kernel(ScriptedParams ep, const uint8_t* __restrict__ records, int rec_bytes, int L,
                                                                   const int32_t* __restrict__ src_index, const int32_t* __restrict__ stop,
                                                                   const int32_t* __restrict__ sel, int32_t* __restrict__ status) {
  extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
  uint32_t* s_st = smem;
  uint8_t* s_mv = reinterpret_cast<uint8_t*>(smem + ep.npl * kWave);
  const int lane = threadIdx.x;
  const int g = blockIdx.x * kWave + lane;   // < Gpad
  const bool mine = g < ep.G && sel[g] == g;
  if (__ballot(mine) == 0ull) return;
  const int P = TP ? TP : ep.P, H = TH ? TH : ep.H;
  const auto ru = RulesOf<V>::make(ep);
  stage_planes(ep, s_st, lane, g);
  const int si = mine ? src_index[g] : -1;   // in [0, n_rec): the prep kernel refused every other index
  for (int i = 0; i < kWave; ++i) {
    const int s = __shfl(si, i);
    if (s < 0) continue;
    const uint8_t* mv = records + (size_t)s * rec_bytes + GR_OFF_MOVES;
    for (int k = lane; k < 2 * L; k += kWave) s_mv[k * kWave + i] = mv[k];
  }
  __syncthreads();
  int target = 0;
  if (mine) {
    const int n_moves = min((int)records[(size_t)si * rec_bytes + GR_OFF_NMOVES], L);
    target = stop ? min(max(stop[g], 0), n_moves) : n_moves;
  }
  Rng rng = rng_open(ep, s_st, lane, g, ST(PL_MISC));
  int played = 0;
  bool going = mine && misc_live(ST(PL_MISC));
#pragma clang loop unroll(disable)
  for (int it = 0; it < L; ++it) {
    bool live = going && played < target && !misc_term(ST(PL_MISC));
    if (__ballot(live) == 0ull) break;
    if (live) {
      const int cur = board_cur(ST(PL_BOARD));
      bool ok = cur >= 0 && cur < P;
      if (ok) {
        const uint32_t pm = ep.shuffle_color ? (ST(PLPERM(cur)) & 0x7fffu) : kIdentityPerm;
        const int m = s_mv[played * kWave + lane], gm = s_mv[(L + played) * kWave + lane];
        const int uid = gr_uid_from_true(m, P, H, ru.C, pm), guid = gr_uid_from_true(gm, P, H, ru.C, pm);
        const uint64_t mask = legal_mask_of<TH>(P, H, ep.A, s_st, lane, cur, pm, ru);
        ok = uid < ep.A - 1 && ((mask >> uid) & 1ull);
        if (ok && ep.sad) ok = guid < ep.A - 1 && ((mask >> guid) & 1ull);
        if (ok)
          for (int p = 0; p < P; ++p) {
            ep.a_out[(size_t)g * P + p] = p == cur ? uid : ep.A - 1;
            ep.g_out[(size_t)g * P + p] = p == cur ? guid : ep.A - 1;
          }
      }
      if (!ok) {
        log_error(ep, g, 8);
        going = false;
        live = false;
      }
    }
    uint32_t greedy_rec = 0;
    float reward = 0.f;
    bool term = false;
    env_logic<1, TP, TH, V>(ep, ep.a_out, ep.g_out, s_st, nullptr, nullptr, lane, g, live, false, rng, greedy_rec, reward, term);
    if (live) ++played;
  }
  if (mine) {
    Refill rf;
    refill_issue(rf, rng, true);
    refill_finish(rf, rng);
    rng_close(rng, s_st, lane);
    for (int p = 0; p < P; ++p)
      ep.legal_bits[(size_t)g * P + p] =
          legal_mask_of<TH>(P, H, ep.A, s_st, lane, p, ep.shuffle_color ? (ST(PLPERM(p)) & 0x7fffu) : kIdentityPerm, ru);
    for (int pl = 0; pl < ep.npl; ++pl) ep.planes[(size_t)pl * ep.Gpad + g] = ST(pl);
    ep.terminal[g] = (uint8_t)misc_term(ST(PL_MISC));
    status[g] = played;
  }
}

typedef void (*EnvPlayoutLoggedFn)(ScriptedParams, const uint8_t*, int, int, const int32_t*, const int32_t*, const int32_t*, int32_t*);
EnvPlayoutLoggedFn pick_playout_logged_kernel(const EnvParams& ep) {
  if (ep.variant) return env_playout_logged_kernel<0, 0, true>;
  if (ep.P == 2 && ep.H == 5) return env_playout_logged_kernel<2, 5, false>;
  return env_playout_logged_kernel<0, 0, false>;
}

}  // namespace

extern "C" {

// shared with csrc/hsad_eval.hip (not part of the public header): what the game log's kernels read of an env
int hsad_internal_env_record_view(const hsad_env* e, GrEnvView* v) {
  if (!e) return set_error(HSAD_ERR_INVALID, "null env");
  if (!e->bound) return set_error(HSAD_ERR_STATE, "hsad_env_bind_outputs must be called first");
  v->planes = e->ep.planes;
  v->deck_hist = e->ep.deck_hist;
  v->G = e->ep.G;
  v->Gpad = e->ep.Gpad;
  v->track_dh = e->ep.track_dh;
  v->deck_max = e->ep.deck_max;
  v->max_life = e->ep.max_life;
  v->bomb = e->ep.bomb;
  v->device = e->device;
  v->ru = rb_rules_of(e->ep);
  return HSAD_OK;
}

int hsad_env_playout_logged(hsad_env* e, const uint8_t* records, int n_rec, const int32_t* src_index, const int32_t* stop, int32_t* status,
                            void* stream) {
  if (!e || !records || !src_index || !status) return set_error(HSAD_ERR_INVALID, "hsad_env_playout_logged: null argument");
  if (!e->bound) return set_error(HSAD_ERR_STATE, "hsad_env_bind_outputs must be called first");
  if (n_rec < 1) return set_error(HSAD_ERR_INVALID, "hsad_env_playout_logged: n_rec must be >= 1");
  const EnvParams& p = e->ep;
  if (p.P > 5 || p.H > 5) return set_error(HSAD_ERR_INVALID, "hsad_env_playout_logged: more than 5 players or 5 cards a hand");
  const int L = gr_capacity(p.P, p.H, p.deck_max, p.max_info, p.nC);
  if (!gr_capacity_ok(L)) return set_error(HSAD_ERR_INVALID, "hsad_env_playout_logged: a game of these rules can have %d moves, a record holds at most 255", L);
  const int rec_bytes = gr_record_bytes(L);
  for (int i = 0; i < n_rec; ++i) {
    const GrHeader h = gr_unpack_header(records + (size_t)i * rec_bytes);
    if (h.version != HSAD_GR_VERSION) return set_error(HSAD_ERR_INVALID, "hsad_env_playout_logged: record %d has version %d, not %d", i, h.version, HSAD_GR_VERSION);
    if (h.P != p.P || h.H != p.H || h.colors != p.nC || h.ranks != p.nR || h.max_info != p.max_info || h.max_life != p.max_life ||
        h.bomb != p.bomb || h.capacity != L)
      return set_error(HSAD_ERR_INVALID, "hsad_env_playout_logged: record %d was played under other rules than the env's", i);
    if (h.n_moves > L || h.n_dealt > 52) return set_error(HSAD_ERR_INVALID, "hsad_env_playout_logged: record %d: n_moves or n_dealt out of range", i);
  }
  const int Gpad = p.Gpad;
  hipStream_t st = (hipStream_t)stream;
  HIP_TRY(hipSetDevice(e->device));
  if (!e->d_sel) HIP_TRY(hipMalloc((void**)&e->d_sel, sizeof(int32_t) * (size_t)Gpad));
  if (!e->script.cards) HIP_TRY(hipMalloc((void**)&e->script.cards, (size_t)Gpad * 52));
  if (!e->script.count) HIP_TRY(hipMalloc((void**)&e->script.count, sizeof(int32_t) * (size_t)Gpad));
  if (!e->d_log_script) HIP_TRY(hipMalloc((void**)&e->d_log_script, (size_t)Gpad * 52));
  if (!e->d_log_count) HIP_TRY(hipMalloc((void**)&e->d_log_count, sizeof(int32_t) * (size_t)Gpad));
  if (!e->d_log_a) HIP_TRY(hipMalloc((void**)&e->d_log_a, 2 * sizeof(int64_t) * (size_t)Gpad * p.P));
  const size_t need = (size_t)n_rec * rec_bytes;
  if (e->d_records_cap < need) {
    HIP_TRY(hipStreamSynchronize(st));   // a replay queued earlier may still read the old buffer
    if (e->d_records) HIP_TRY(hipFree(e->d_records));
    e->d_records = nullptr;
    e->d_records_cap = 0;
    HIP_TRY(hipMalloc((void**)&e->d_records, need));
    e->d_records_cap = need;
  }
  const size_t lds = sizeof(uint32_t) * (size_t)p.npl * kWave + 2 * (size_t)L * kWave;
  const void* fn = reinterpret_cast<const void*>(pick_playout_logged_kernel(p));
  HIP_TRY(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  if (!e->scripted) {   // the first script since creation / reset: no game has one yet (hsad_env_rewind_scripted)
    HIP_TRY(hipMemsetAsync(e->script.cards, 0, (size_t)Gpad * 52, st));
    HIP_TRY(hipMemsetAsync(e->script.count, 0, sizeof(int32_t) * (size_t)Gpad, st));
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(pick_scripted_step_kernel(p.P, p.H, p.variant != 0)),
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)e->lds_bytes));
    e->scripted = true;
  }
  HIP_TRY(hipMemcpyAsync(e->d_records, records, need, hipMemcpyHostToDevice, st));
  hipLaunchKernelGGL(env_logged_prep_kernel, dim3((p.G + 255) / 256), dim3(256), 0, st, p, e->d_records, n_rec, rec_bytes, src_index,
                     e->d_log_script, e->d_log_count, status);
  hipLaunchKernelGGL(env_rewind_kernel, dim3((p.G + 255) / 256), dim3(256), 0, st, p, e->script, e->d_log_script, e->d_log_count, e->d_sel);
  ScriptedParams sp;
  static_cast<EnvParams&>(sp) = p;
  sp.sc = e->script;
  sp.n_iter = 1;
  sp.a_out = e->d_log_a;
  sp.g_out = e->d_log_a + (size_t)Gpad * p.P;
  sp.dbg = nullptr;
  hipLaunchKernelGGL(pick_playout_logged_kernel(p), dim3(Gpad / kWave), dim3(kWave), lds, st, sp, e->d_records, rec_bytes, L, src_index, stop,
                     e->d_sel, status);
  HIP_TRY(hipGetLastError());
  ObserveArgs oa;
  oa.sel = e->d_sel;
  oa.sel_limit = p.G;
  oa.sad_bits = nullptr;   // rebuilding the SAD section from a record is out of scope: all-zero, as after hsad_env_import_state
  oa.sad_f32 = nullptr;
  oa.sad_words = nullptr;
  oa.sad_pw64 = 0;
  return launch_observe(e, oa, st);
}

}  // extern "C"
