// hsad_game_log.inc — the device log of a tournament's games and the way out of it (include/hsad.h: hsad_game_log_*): append one
// move per live game, select the finished games a filter keeps (stable compaction), gather their records.  Textually part of
// hsad_eval.hip (included at its end: it uses that file's error helpers and sits next to hsad_seating_behaviour, whose call site
// is its own).  Layout and bit definitions: csrc/hsad_game_record.h.
//
// All three stream bytes once.  The planes are time-major [L][Gpad]: the lanes of a wave are consecutive games, so an append
// writes and the filter's flag scan reads consecutive bytes.  No atomics except the overflow counter.

#include "hsad_game_record.h"

extern "C" int hsad_internal_env_record_view(const hsad_env* e, GrEnvView* v);

struct hsad_game_log {
  int device, G, Gpad, L, P;
  uint8_t* planes;        // move | greedy | flags, each [L][Gpad]
  int32_t* n_moves;       // [Gpad]
  uint32_t* overflow;     // [1]
  uint8_t* keep;          // [Gpad] select's predicate, between its launches
  int32_t* block_count;   // [Gpad / kGlThreads + 1] select's per-workgroup counts, then offsets
};

namespace {

constexpr int kGlThreads = 256;

__global__ __launch_bounds__(kGlThreads) void game_log_append_kernel(GrEnvView v, int L, uint8_t* __restrict__ planes,
                                                                     int32_t* __restrict__ n_moves, uint32_t* __restrict__ overflow,
                                                                     const int64_t* __restrict__ a, const int64_t* __restrict__ ga) {
  const int g = blockIdx.x * kGlThreads + threadIdx.x;
  if (g >= v.G) return;
  const GlobalPlanes w{v.planes, (size_t)v.Gpad, g};
  const uint32_t misc = w(PL_MISC);
  if (!misc_live(misc)) return;
  const RbRules& ru = v.ru;
  const int P = ru.P;
  const int p = board_cur(w(PL_BOARD));
  if (p < 0 || p >= P) return;
  const int64_t uid = a[(size_t)g * P + p];
  if (uid < 0 || uid >= (int64_t)(ru.A - 1)) return;
  int64_t guid = ga ? ga[(size_t)g * P + p] : uid;
  if (guid < 0 || guid >= (int64_t)(ru.A - 1)) guid = uid;
  const int k = misc_num_step(misc);
  if (k >= L) {
    atomicAdd(overflow, 1u);
    return;
  }
  const uint32_t perm = ru.shuffle_color ? (w(PLPERM(p)) & 0x7fffu) : kGrIdentityPerm;
  const size_t plane = (size_t)L * v.Gpad, at = (size_t)k * v.Gpad + g;
  planes[at] = (uint8_t)gr_uid_to_true((int)uid, P, ru.H, ru.nC, perm);
  planes[plane + at] = (uint8_t)gr_uid_to_true((int)guid, P, ru.H, ru.nC, perm);
  planes[2 * plane + at] = gr_flags(bh_classify(w, ru, p, uid));
  n_moves[g] = k + 1;
}

// does game g pass?  The result fields are read the way the gather writes them.
__device__ __forceinline__ bool game_log_keeps(const GrEnvView& v, int L, const uint8_t* __restrict__ planes, const int32_t* __restrict__ n_moves,
                                               const hsad_game_filter& f, const uint8_t* __restrict__ take, int g) {
  const GlobalPlanes w{v.planes, (size_t)v.Gpad, g};
  const uint32_t misc = w(PL_MISC), board = w(PL_BOARD);
  const int end = gr_end_reason(board, misc, v.ru.nC, v.ru.nR);
  if (end == HSAD_GR_END_UNFINISHED) return false;
  if (take && !take[g]) return false;
  const int n = min(n_moves[g], L);
  bool hit = false;
  if (f.flag_mask) {
    const uint8_t* fl = planes + 2 * (size_t)L * v.Gpad + g;
    const uint32_t seats = f.seat_mask ? (uint32_t)f.seat_mask : 0xffffffffu;
    int seat = 0;
    for (int k = 0; k < n; ++k) {
      if (((seats >> seat) & 1u) && (fl[(size_t)k * v.Gpad] & (uint32_t)f.flag_mask)) hit = true;
      if (++seat == v.ru.P) seat = 0;
    }
  }
  return gr_filter_pass(f, gr_score(board, misc, v.bomb), board_life(board), n, end, hit);
}

// ---- select: count per workgroup, scan the counts, write ----------------------------------------------------------------------------
__global__ __launch_bounds__(kGlThreads) void game_log_count_kernel(GrEnvView v, int L, const uint8_t* __restrict__ planes,
                                                                    const int32_t* __restrict__ n_moves, hsad_game_filter f,
                                                                    const uint8_t* __restrict__ take, uint8_t* __restrict__ keep,
                                                                    int32_t* __restrict__ block_count) {
  __shared__ int s_wave[kGlThreads / 64];
  const int t = threadIdx.x, g = blockIdx.x * kGlThreads + t;
  const bool k = g < v.G && game_log_keeps(v, L, planes, n_moves, f, take, g);
  if (g < v.Gpad) keep[g] = k ? 1 : 0;
  const int c = __popcll(__ballot(k));
  if ((t & 63) == 0) s_wave[t >> 6] = c;
  __syncthreads();
  if (t == 0) {
    int s = 0;
    for (int i = 0; i < kGlThreads / 64; ++i) s += s_wave[i];
    block_count[blockIdx.x] = s;
  }
}

// one workgroup: block_count[0 .. nb) -> its exclusive prefix sums, *n_out = the total.  Chunks of kGlThreads counts, in order.
__global__ __launch_bounds__(kGlThreads) void game_log_scan_kernel(int32_t* __restrict__ block_count, int nb, int32_t* __restrict__ n_out) {
  __shared__ int s_val[kGlThreads];
  const int t = threadIdx.x;
  int base = 0;
  for (int b0 = 0; b0 < nb; b0 += kGlThreads) {
    const int mine = b0 + t < nb ? block_count[b0 + t] : 0;
    s_val[t] = mine;
    __syncthreads();
    for (int d = 1; d < kGlThreads; d <<= 1) {   // inclusive scan, Hillis-Steele
      const int add = t >= d ? s_val[t - d] : 0;
      __syncthreads();
      s_val[t] += add;
      __syncthreads();
    }
    if (b0 + t < nb) block_count[b0 + t] = base + s_val[t] - mine;
    const int total = s_val[kGlThreads - 1];
    __syncthreads();
    base += total;
  }
  if (t == 0) *n_out = base;
}

__global__ __launch_bounds__(kGlThreads) void game_log_write_kernel(int G, const uint8_t* __restrict__ keep,
                                                                    const int32_t* __restrict__ block_off, int32_t* __restrict__ index_out) {
  __shared__ int s_wave[kGlThreads / 64];
  const int t = threadIdx.x, g = blockIdx.x * kGlThreads + t;
  const bool k = g < G && keep[g];
  const uint64_t b = __ballot(k);
  if ((t & 63) == 0) s_wave[t >> 6] = __popcll(b);
  __syncthreads();
  int before = block_off[blockIdx.x];
  for (int i = 0; i < (t >> 6); ++i) before += s_wave[i];
  before += __popcll(b & ((1ull << (t & 63)) - 1ull));
  if (k) index_out[before] = g;   // before < the number of kept games <= G
}

// ---- gather: one wave per record ----------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kGlThreads) void game_log_gather_kernel(GrEnvView v, int L, const uint8_t* __restrict__ planes,
                                                                     const int32_t* __restrict__ n_moves, const int32_t* __restrict__ index,
                                                                     int n, uint8_t* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int j = blockIdx.x * (kGlThreads / 64) + (threadIdx.x >> 6);
  if (j >= n) return;
  const int bytes = gr_record_bytes(L);
  uint8_t* o = out + (size_t)j * bytes;
  const int g = index[j];
  if (g < 0 || g >= v.G) {
    for (int i = lane; i < bytes; i += 64) o[i] = 0;
    return;
  }
  const GlobalPlanes w{v.planes, (size_t)v.Gpad, g};
  const uint32_t misc = w(PL_MISC), board = w(PL_BOARD);
  const int nm = misc_started(misc) ? min(n_moves[g], L) : 0;
  const int nd = misc_started(misc) ? v.deck_max - misc_deck_size(misc) : 0;
  if (lane == 0) {
    GrHeader h;
    h.version = HSAD_GR_VERSION;
    h.P = v.ru.P;
    h.H = v.ru.H;
    h.colors = v.ru.nC;
    h.ranks = v.ru.nR;
    h.max_info = v.ru.max_info;
    h.max_life = v.max_life;
    h.bomb = v.bomb;
    h.n_moves = nm;
    h.n_dealt = nd;
    h.score = gr_score(board, misc, v.bomb);
    h.lives = board_life(board);
    h.info = board_info(board);
    h.end = gr_end_reason(board, misc, v.ru.nC, v.ru.nR);
    h.capacity = L;
    gr_pack_header(h, o);
  }
  if (lane < 52) o[GR_OFF_DECK + lane] = lane < nd ? v.deck_hist[(size_t)g * 52 + lane] : (uint8_t)0;
  const size_t plane = (size_t)L * v.Gpad;
  for (int i = lane; i < 3 * L; i += 64) {
    const int q = i / L, k = i - q * L;
    o[GR_OFF_MOVES + i] = k < nm ? planes[q * plane + (size_t)k * v.Gpad + g] : (uint8_t)0;
  }
}

int log_view(const char* who, const hsad_game_log* log, const hsad_env* env, GrEnvView* v) {
  if (!log || !env) return efail(HSAD_ERR_INVALID, "%s: null argument", who);
  CK(hsad_internal_env_record_view(env, v));
  if (v->G != log->G || v->Gpad != log->Gpad || v->ru.P != log->P || v->device != log->device ||
      gr_capacity(v->ru.P, v->ru.H, v->deck_max, v->ru.max_info, v->ru.nC) != log->L)
    return efail(HSAD_ERR_INVALID, "%s: the log was made for an env of other sizes or rules", who);
  if (!v->track_dh) return efail(HSAD_ERR_STATE, "%s: the env does not track its deck history", who);
  return HSAD_OK;
}

}  // namespace

extern "C" {

int64_t hsad_game_record_bytes(const hsad_env* env) {
  GrEnvView v;
  if (!env || hsad_internal_env_record_view(env, &v)) return 0;
  return gr_record_bytes(gr_capacity(v.ru.P, v.ru.H, v.deck_max, v.ru.max_info, v.ru.nC));
}

void hsad_game_log_destroy(hsad_game_log* log) {
  if (!log) return;
  (void)hipSetDevice(log->device);
  if (log->planes) (void)hipFree(log->planes);
  if (log->n_moves) (void)hipFree(log->n_moves);
  if (log->overflow) (void)hipFree(log->overflow);
  if (log->keep) (void)hipFree(log->keep);
  if (log->block_count) (void)hipFree(log->block_count);
  delete log;
}

int hsad_game_log_create(const hsad_env* env, hsad_game_log** out) {
  if (!env || !out) return efail(HSAD_ERR_INVALID, "hsad_game_log_create: null argument");
  GrEnvView v;
  CK(hsad_internal_env_record_view(env, &v));
  if (!v.track_dh) return efail(HSAD_ERR_STATE, "hsad_game_log_create: the env does not track its deck history (a record needs the deal)");
  if (v.ru.P > kBhMaxPlayers) return efail(HSAD_ERR_INVALID, "hsad_game_log_create: %d players, at most %d", v.ru.P, kBhMaxPlayers);
  const int L = gr_capacity(v.ru.P, v.ru.H, v.deck_max, v.ru.max_info, v.ru.nC);
  if (!gr_capacity_ok(L)) return efail(HSAD_ERR_INVALID, "hsad_game_log_create: a game of these rules can have %d moves, a log holds at most 255", L);
  hsad_game_log* log = new hsad_game_log();
  log->device = v.device;
  log->G = v.G;
  log->Gpad = v.Gpad;
  log->L = L;
  log->P = v.ru.P;
  const int nb = (v.Gpad + kGlThreads - 1) / kGlThreads + 1;
  hipError_t he = hipSetDevice(v.device);
  if (he == hipSuccess) he = hipMalloc((void**)&log->planes, 3 * (size_t)L * v.Gpad);
  if (he == hipSuccess) he = hipMalloc((void**)&log->n_moves, sizeof(int32_t) * (size_t)v.Gpad);
  if (he == hipSuccess) he = hipMalloc((void**)&log->overflow, sizeof(uint32_t));
  if (he == hipSuccess) he = hipMalloc((void**)&log->keep, (size_t)v.Gpad);
  if (he == hipSuccess) he = hipMalloc((void**)&log->block_count, sizeof(int32_t) * (size_t)nb);
  if (he == hipSuccess) he = hipMemset(log->planes, 0, 3 * (size_t)L * v.Gpad);
  if (he == hipSuccess) he = hipMemset(log->n_moves, 0, sizeof(int32_t) * (size_t)v.Gpad);
  if (he == hipSuccess) he = hipMemset(log->overflow, 0, sizeof(uint32_t));
  if (he != hipSuccess) {
    hsad_game_log_destroy(log);
    return efail(HSAD_ERR_NOMEM, "hsad_game_log_create: %s", hipGetErrorString(he));
  }
  *out = log;
  return HSAD_OK;
}

int hsad_game_log_clear(hsad_game_log* log, void* stream) {
  if (!log) return efail(HSAD_ERR_INVALID, "hsad_game_log_clear: null log");
  hipStream_t st = (hipStream_t)stream;
  HIP_TRY(hipMemsetAsync(log->planes, 0, 3 * (size_t)log->L * log->Gpad, st));
  HIP_TRY(hipMemsetAsync(log->n_moves, 0, sizeof(int32_t) * (size_t)log->Gpad, st));
  HIP_TRY(hipMemsetAsync(log->overflow, 0, sizeof(uint32_t), st));
  return HSAD_OK;
}

int hsad_game_log_capacity(const hsad_game_log* log) { return log ? log->L : 0; }

int hsad_game_log_overflow_count(hsad_game_log* log, int32_t* count) {
  if (!log || !count) return efail(HSAD_ERR_INVALID, "hsad_game_log_overflow_count: null argument");
  uint32_t h = 0;
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(&h, log->overflow, sizeof(h), hipMemcpyDeviceToHost));
  *count = (int32_t)h;
  return HSAD_OK;
}

int hsad_game_log_append(hsad_game_log* log, const hsad_env* env, const int64_t* a, const int64_t* greedy_a, void* stream) {
  GrEnvView v;
  CK(log_view("hsad_game_log_append", log, env, &v));
  if (!a) return efail(HSAD_ERR_INVALID, "hsad_game_log_append: action tensor is null");
  hipLaunchKernelGGL(game_log_append_kernel, dim3((v.G + kGlThreads - 1) / kGlThreads), dim3(kGlThreads), 0, (hipStream_t)stream, v, log->L,
                     log->planes, log->n_moves, log->overflow, a, greedy_a);
  HIP_TRY(hipGetLastError());
  return HSAD_OK;
}

int hsad_game_log_select(hsad_game_log* log, const hsad_env* env, const hsad_game_filter* filter, const uint8_t* take,
                         int32_t* index_out, int32_t* n_out, void* stream) {
  GrEnvView v;
  CK(log_view("hsad_game_log_select", log, env, &v));
  if (!index_out || !n_out) return efail(HSAD_ERR_INVALID, "hsad_game_log_select: null output");
  hsad_game_filter f = {0, 255, 255, 0, 255, 0, 0, 0};   // every finished game
  if (filter) f = *filter;
  const int nb = (v.G + kGlThreads - 1) / kGlThreads;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(game_log_count_kernel, dim3(nb), dim3(kGlThreads), 0, st, v, log->L, log->planes, log->n_moves, f, take, log->keep,
                     log->block_count);
  hipLaunchKernelGGL(game_log_scan_kernel, dim3(1), dim3(kGlThreads), 0, st, log->block_count, nb, n_out);
  hipLaunchKernelGGL(game_log_write_kernel, dim3(nb), dim3(kGlThreads), 0, st, v.G, log->keep, log->block_count, index_out);
  HIP_TRY(hipGetLastError());
  return HSAD_OK;
}

int hsad_game_log_gather(hsad_game_log* log, const hsad_env* env, const int32_t* index, int n, uint8_t* out, void* stream) {
  GrEnvView v;
  CK(log_view("hsad_game_log_gather", log, env, &v));
  if (n < 0 || (n > 0 && (!index || !out))) return efail(HSAD_ERR_INVALID, "hsad_game_log_gather: n < 0 or a null argument");
  if (n == 0) return HSAD_OK;
  const int per = kGlThreads / 64;
  hipLaunchKernelGGL(game_log_gather_kernel, dim3((n + per - 1) / per), dim3(kGlThreads), 0, (hipStream_t)stream, v, log->L, log->planes,
                     log->n_moves, index, n, out);
  HIP_TRY(hipGetLastError());
  return HSAD_OK;
}

}  // extern "C"
