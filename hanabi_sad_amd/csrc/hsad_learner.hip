// hsad_learner.hip — the learner of the composite boundary (include/hsad.h: hsad_r2d2_learner_*, hsad_r2d2_loss_fwd / _loss_bwd /
// _optimizer_step / _sync_target_with_online): loss forward (online + target net), BPTT, clip + Adam (pyhanabi/selfplay.py:208-244,
// r2d2.py:383-499).  The whole kernel schedule of an update lives here behind plain pointers: plan_update() resolves ONCE what runs (forward
// and backward kind, chunk boundaries, the stages of the fused BPTT launch, grouped weight gradients), loss_fwd / loss_bwd are lists of stage
// functions that read that plan, and FwdHandoff is everything the backward half continues from.  The kernels are the ones in hsad_r2d2.hip.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <vector>

#include "hsad_agent_internal.h"

// hsad_loss_tail with a buffer the launch clears on the side (csrc/hsad_r2d2.hip)
extern "C" int hsad_internal_loss_tail(const float* heads, const float* heads_t, int ldh, const float* legal, const float* q_online, const float* online_qa,
                                       const float* block_min, int n_block_min, const float* reward, const float* bootstrap, const float* seq_len,
                                       const float* weight, const float* own_hand, const int64_t* action, int T, int B, int A, int NP, int multi_step,
                                       double gamma, float pred_weight, int64_t* greedy, float* target_qa, float* err, float* priority, float* loss,
                                       float* xent_sum, float* dqa, void* dheads16, int ldo, float* zero_buf, int64_t zero_n, const void* WT16, float* dO32,
                                       int H, void* stream);
// both head layers + the online dueling head as one launch (csrc/hsad_r2d2.hip, heads_q_kernel)
extern "C" int hsad_internal_heads_q_supported(int M, int H, int NH, int A, const void* legal, const void* q, const void* heads, const void* heads_t);
extern "C" int hsad_internal_heads_q(const void* o16, const void* o16_t, const void* W16, const void* W16_t, const float* bias, const float* bias_t, int M,
                                     int H, int NH, int A, float* heads, float* heads_t, const float* legal, const int64_t* action, float* q, float* qa,
                                     float* block_min, void* stream);

namespace {

// tiny elementwise helpers of the learner
__global__ void repeat_players_kernel(const float* __restrict__ x, int n_in, int P, float* __restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n_in * P) out[i] = x[i / P];
}
__global__ void axpy_kernel(float* __restrict__ y, const float* __restrict__ x, float a, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) y[i] += a * x[i];
}
extern "C" {      // (these two keep the unmangled names they have always had in a kernel trace)
// d mean_b(weight_b loss_b) / d online_qa from the TD errors of the last forward pass, for weights that arrive AFTER it (same arithmetic
// as td_loss_kernel / loss_tail_kernel: -clamp(err, -1, 1) * mask * weight / B)
__global__ void dqa_reweight_kernel(const float* __restrict__ err, const float* __restrict__ seq_len, const float* __restrict__ weight, int T, int B,
                                    float* __restrict__ dqa) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= T * B) return;
  const int t = i / B, b = i - t * B;
  const float mask = (float)t < seq_len[b] ? 1.f : 0.f;
  const float g = fminf(fmaxf(err[i], -1.f), 1.f);
  dqa[i] = -g * mask * weight[b] / (float)B;
}
struct TimeoutWords {
  const unsigned* p[40];
  int n;
};
__global__ void timeout_gather_kernel(TimeoutWords w, unsigned* host_flag) {      // one lane per word (40 dependent loads in one thread took 12 us)
  const unsigned v = (int)threadIdx.x < w.n ? w.p[threadIdx.x][0] : 0u;
  if (v) __hip_atomic_store(host_flag, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}
}  // extern "C"

// events that only order device work between the learner's two streams: device-scope release (developer switch HSAD_EVENT_SYSTEM=1: the
// runtime's default)
unsigned learner_event_flags() {
  static const unsigned f = hipEventDisableTiming | ((getenv("HSAD_EVENT_SYSTEM") && atoi(getenv("HSAD_EVENT_SYSTEM"))) ? 0u : (unsigned)hipEventReleaseToDevice);
  return f;
}

enum { kPlain = 0, kPipelined = 1, kFused = 2 };      // hsad_learner_plan.fwd_kind / .bwd_kind

// What an update runs, resolved by plan_update() from the stored flags (set_fused, set_schedule) and the shape.  Every stage reads this.
struct LearnerPlan {
  int fwd_kind = -1;        // (-1: no loss_fwd yet)
  bool pipe;                // multi-recurrence persistent launches + weight gradients on the side stream are possible at this shape
  int fwd_nets, fwd_layers; // fused forward: nets and stacked layers per launch
  int fwd_chunks;           // time chunks of the chunk-pipelined schedule (also the chunk length its counter blocks are laid out for)
  int bwd_kind, bptt_chunks;
  int cut[9], layout_steps; // fused BPTT: chunk c = steps [cut[c], cut[c + 1]); the longest chunk lays out the counter blocks
  bool use_split, use_proj, use_sink;      // fused BPTT: the stages that were asked for AND whose 16-workgroup groups fit the chip
  bool dgt_in_kernel;       // ... the launch writes dG transposed and the LSTM bias gradients itself
  bool group;               // ... and every weight gradient behind it is ONE grouped split-K launch
  bool chunk_input;         // chunked fused BPTT: a chunk's share of the input layer's backward pass runs on the side stream, too
  bool wide_blocks;         // the 16-row x 64-unit blocking, as asked of the launcher (it takes it where the shape allows)
  int heads_split;          // K split of the heads' weight gradient
  int counter_sets() const { return use_split ? (use_proj ? (use_sink ? 8 : 6) : 4) : 2; }      // counter sets per row block of a fused BPTT launch
};

// the arguments of a loss_fwd (own_hand: NULL unless pred_weight > 0)
struct LossArgs {
  const float *legal, *reward, *bootstrap, *seq_len, *own_hand, *weight;
  const int64_t* a;
  int num_player;
  float pred_weight, *loss, *priority;
  bool want_grad;
};

// What loss_fwd hands to loss_bwd: written once at its exit, consumed at the top of loss_bwd
struct FwdHandoff {
  bool have_fwd = false;
  LearnerPlan plan;               // what that loss_fwd ran (fused forward: gates / cseq are stored fragment-major); loss_bwd re-resolves its backward half
  bool pre_T = false;             // the transposes of the forward activations are already issued on the side stream
  bool one_launch_heads = false;  // both head layers + the online dueling head ran as one launch
  bool dheads_ready = false;      // the loss tail already produced d loss / d heads
  bool dO_ready = false;          // ... and d loss / d o of the top layer
  bool dc01_zero = false;         // ... and cleared dc[0], dc[1] (contiguous)
  bool clone = false;             // the forward was hsad_r2d2_clone_fwd: no TD errors to re-weight
  LossArgs batch{};               // the caller's batch (must still be alive)
};

}  // namespace

struct hsad_r2d2_learner {
  hsad_r2d2_net *on, *tg;
  int T, B, M, multi_step, n_cu, step_count = 0;
  double gamma;
  float lr, adam_eps, clip;
  int wgrad_split = 8, chunks = 4;      // hsad_r2d2_learner_set_schedule
  // hsad_r2d2_learner_set_fused, as asked for (include/hsad.h has the bit table); plan_update() decides what the shape allows
  int fused_fwd = 1, fused_bwd = 1;
  int bchunks = 1;            // (measured: 1 chunk 1.57 ms, 2 chunks 1.61, 4 chunks 1.78 per update)
  int btail = 0;
  bool split_bptt = true, proj_bptt = true, sink_bptt = true, dgt_in_kernel = true, group_wgrad = true, wide_bptt = true, fuse_heads = true;
  bool split_refresh = false; // (measured 1.521 vs 1.504 ms per update in line -- the refresh slows the input-layer GEMM it runs next to by more than it hides)
  FwdHandoff hand;
  hipEvent_t ev_ck[8] = {};
  unsigned* fbsync[2];        // ping-pong counter blocks of the fused BPTT launches (up to 8 counter sets x up to T steps)
  int fbflip = 0, fb_tc = 0, fb_sets = 2;      // ... and the layout they are in use with: chunk length, LearnerPlan::counter_sets()
  size_t fbsync_words;
  int group_split_l = 3, group_split_in = 8;     // K ranges per LSTM problem / of the input layer's: (4 x 16 tiles) x 3 + 8 tiles x 8 = one item per CU
  float* group_ws = nullptr;
  int64_t group_ws_floats = 0;
  volatile unsigned* h_timeout = nullptr;      // pinned, device-mapped: OR of the sticky timeout words as of the last gathered update (timeout_gather_kernel)
  unsigned* d_timeout = nullptr;               // its device address
  bool gflat_zero = true;     // the gradient buffer is all zero (creation; optimizer_step clears it behind Adam, as optim.zero_grad() does)
  unsigned* fsync[3][2];      // ping-pong counter blocks of the fused launches: [log2(recurrences per launch)][flip]
  int fflip[3] = {0, 0, 0};
  size_t fsync_words[3];
  Buf arena, opt, sync_buf;
  float *gflat, *m, *v, *osc;
  hipStream_t side = nullptr;
  hipEvent_t ev_a = nullptr, ev_b = nullptr, ev_c = nullptr, ev_d = nullptr, ev_e = nullptr;
  // activations (q = 0 online, 1 target).  xin = the LSTM's input = the last layer of the input MLP (x1, or x2 with two fc layers)
  bf16_t *a16, *x1[2], *x2[2], *xin[2], *hseq[2][kMaxL], *xchg_f[2][kMaxL], *zero16, *sc16;
  const bf16_t* a16_in = nullptr;  // the input operand of the update in flight: a16 (cast here) or the caller's bf16 batch
  float *gates[2][kMaxL], *cseq[2][kMaxL], *hT[2][kMaxL], *czero;
  float *heads, *heads_t, *q, *qa, *tqa, *qa_s, *tqa_s, *err, *dqa, *dqa_r, *w_r, *xs, *qscratch;
  int64_t* greedy;
  // backward
  bf16_t *dheads, *dG[kMaxL], *dx1, *dx2, *hsT[kMaxL], *hpT[kMaxL], *x1T, *x2T, *a16T, *dGT, *dx1T, *dx2T, *dheadsT, *xchg_b[kMaxL], *xout_b = nullptr, *xout_b2 = nullptr;
  int Mp;                 // contraction length of the weight-gradient GEMMs: M padded to the GEMM's K tile (64)
  float *dO[kMaxL], *dc[kMaxL], *wgrad_ws, *wgrad_ws2, *heads_ws;
  bf16_t* dGT2;           // second transposed-gradient operand: layer 0's weight gradients on the main stream next to layer 1's on the side stream
  // ping-pong counter blocks of the persistent launches: [kind fwd/bwd][nrec - 1][flip]
  unsigned* sync[2][4][2];
  int flip[2][4];
  unsigned* sync1;        // unchunked single-recurrence launches (the kernels zero it themselves)
  size_t sync_words[2][4];
};

namespace {

inline int nrb_of(int B) { return (B + 31) / 32; }

struct Shape {
  int T, B, M, Mp, H, H4, A, NH, NHp, F, Fp, NP, NL, nfc;
};
Shape shape_of(const hsad_r2d2_learner* L) {
  const hsad_r2d2_net* n = L->on;
  return {L->T, L->B, L->M, L->Mp, n->H, 4 * n->H, n->A, n->NH, n->NHp, n->F, n->Fp, n->NP, n->L, n->nfc};
}

// Forward half of the plan.  Persistent multi-recurrence launches + the shared delayed-copy operand of the weight gradients need H in
// {256, 512}, at most 512 rows, rows a multiple of 8 and T * rows a multiple of the GEMM K tile; the layer pipeline is written for two LSTM
// layers; everything else takes the unchunked (plain) schedule.  Fused forward (persistent launches over the whole sequence): a (net, row
// block)'s layers x H/32 workgroups must share an XCD (one workgroup per CU).
// nets: how many nets the forward runs (2: online + target, the TD loss; 1: the online net alone, cloning).
void plan_forward(const hsad_r2d2_learner* L, LearnerPlan& P, int nets) {
  const Shape d = shape_of(L);
  const int T = d.T, B = d.B, H = d.H, nrb = nrb_of(B);
  P.pipe = d.NL == 2 && (H == 256 || H == 512) && B <= 512 && B % 8 == 0 && d.M % 64 == 0;
  P.fwd_chunks = P.pipe ? L->chunks : 1;
  while (P.fwd_chunks > 1 && (T % P.fwd_chunks || ((T / P.fwd_chunks) * B) % 64)) --P.fwd_chunks;
  P.fwd_nets = P.fwd_layers = 0;
  // (T < 2: a one-step "sequence" has no recurrence to fuse -- the fused forward launch faulted on it, found in round 6; the chunked schedule runs it)
  if (L->fused_fwd && T >= 2 && (H == 256 || H == 512) && B % 32 == 0 && (size_t)T * B * H * 16 < (1ull << 32))
    for (int g = std::min(d.NL, 2); g >= 1 && !P.fwd_nets; --g)
      for (int nn = nets; nn >= 1 && !P.fwd_nets; --nn)
        if (g * (H / 32) * ((nn * nrb + 7) / 8) <= L->n_cu / 8) P.fwd_nets = nn, P.fwd_layers = g;
  P.fwd_kind = P.fwd_nets ? kFused : P.pipe ? kPipelined : kPlain;
}

// Backward half, given the forward that ran (P.fwd_kind, P.fwd_chunks): loss_bwd resolves it again under the flags in force then.
void plan_bptt(const hsad_r2d2_learner* L, LearnerPlan& P) {
  const Shape d = shape_of(L);
  const int T = d.T, B = d.B, H = d.H;
  P.use_split = P.use_proj = P.use_sink = P.dgt_in_kernel = P.group = P.chunk_input = P.wide_blocks = false;
  P.layout_steps = 0;
  // (NH = A + 1 + 3 hand rows: one row tile -- four column tiles x split; a deeper split than the big weight gradients' fills more CUs:
  // 30 -> 18 us, and with it the whole side-stream chain behind the BPTT launch starts earlier: 1.385 -> 1.362 ms per update)
  P.heads_split = (d.Mp % (64 * 4 * L->wgrad_split) == 0) ? 4 * L->wgrad_split : L->wgrad_split;
  int nbc = L->bchunks;
  while (nbc > 1 && (T % nbc || ((T / nbc) * B) % 64)) --nbc;
  const bool fused = P.pipe && L->fused_bwd && P.fwd_kind == kFused && B % 32 == 0 && 2 * (H / 32) * ((nrb_of(B) + 7) / 8) <= L->n_cu / 8 && nbc <= 8;
  P.bwd_kind = fused ? kFused : P.pipe ? kPipelined : kPlain;
  P.bptt_chunks = fused ? nbc : P.pipe ? P.fwd_chunks : 1;
  if (!fused) return;
  // equal chunks, or (btail) a long chunk [tail, T) first and the short head [0, tail) last: the long chunk's weight gradients hide behind the
  // head's recurrence and only the head's (and the input layer's) are left for the tail of the update
  const int tail = (L->btail > 0 && L->btail < T) ? L->btail : 0;
  if (tail) P.bptt_chunks = nbc = 2;
  for (int c = 0; c <= nbc; ++c) P.cut[c] = tail ? (c == 0 ? 0 : c == 1 ? tail : T) : c * (T / nbc);
  for (int c = 0; c < nbc; ++c) P.layout_steps = std::max(P.layout_steps, P.cut[c + 1] - P.cut[c]);
  // split placement / projection / sink stage only when their 16-workgroup groups (2 / 3 / 4 per row block) fit the chip
  P.use_split = L->split_bptt && nrb_of(B) * 2 * (H / 32) <= L->n_cu;
  P.use_proj = P.use_split && L->proj_bptt && nrb_of(B) * 3 * (H / 32) <= L->n_cu;
  P.use_sink = P.use_proj && L->sink_bptt && nrb_of(B) * 4 * (H / 32) <= L->n_cu;
  // one chunk: the launch writes dG transposed (and the bias gradients) itself -- no transpose passes in the tail of the update.  The
  // row-major dG is not written then, so this needs the sink stage (otherwise the input layer's backward GEMM reads dG0 row-major)
  P.dgt_in_kernel = nbc == 1 && L->dgt_in_kernel && P.use_sink;
  P.group = P.dgt_in_kernel && d.nfc == 1 && L->group_wgrad && (d.H4 % 256) == 0 && (H % 256) == 0 && (d.Mp % 128) == 0 && (d.Fp % 4) == 0;
  P.chunk_input = d.nfc == 1 && nbc > 1 && d.M % 4 == 0 && H % 4 == 0 && L->wgrad_split > 1;
  P.wide_blocks = L->wide_bptt && P.dgt_in_kernel;
}

// pure: no HIP call, no write to L
LearnerPlan plan_update(const hsad_r2d2_learner* L, int nets = 2) {
  LearnerPlan P{};
  plan_forward(L, P, nets);
  plan_bptt(L, P);
  return P;
}

// one arena for every activation of an update.  Hand-off buffers are sized for the longest chunk any schedule can ask for (chunks = 1:
// Tc = T), so that hsad_r2d2_learner_set_schedule may change the chunk count of an existing learner
int learner_alloc_arena(hsad_r2d2_learner* L) {
  const hsad_r2d2_net* online = L->on;
  const size_t T = L->T, M = L->M, B = L->B, H = online->H, H4 = 4 * H, Fp = online->Fp, NH = online->NH, NHp = online->NHp, A = online->A, Mp = L->Mp;
  const int NL = online->L, nfc = online->nfc;
  const bool pipe0 = plan_update(L).pipe;
  const size_t nrb = nrb_of((int)B), xf = T * nrb * 32 * H, xb = T * nrb * 32 * H4;
  std::vector<std::pair<void**, size_t>> slots;
  auto want = [&](auto** pp, size_t bytes) { slots.push_back({reinterpret_cast<void**>(pp), (bytes + 255) & ~(size_t)255}); };
  want(&L->a16, M * Fp * 2);
  for (int q = 0; q < 2; ++q) {
    want(&L->x1[q], M * H * 2);
    if (nfc == 2) want(&L->x2[q], M * H * 2);
    for (int l = 0; l < NL; ++l) {
      want(&L->gates[q][l], M * H4 * 4);
      want(&L->hseq[q][l], M * H * 2);
      want(&L->cseq[q][l], M * H * 4);
      want(&L->hT[q][l], B * H * 4);
      want(&L->xchg_f[q][l], pipe0 ? xf * 2 : 256);
    }
  }
  want(&L->zero16, B * H * 2);
  want(&L->sc16, B * H * 2);
  want(&L->czero, B * H * 4);
  want(&L->heads, M * NH * 4);
  want(&L->heads_t, M * NH * 4);
  want(&L->q, M * A * 4);
  for (float** pp : {&L->qa, &L->tqa, &L->qa_s, &L->tqa_s, &L->err, &L->dqa, &L->dqa_r}) want(pp, M * 4);
  for (float** pp : {&L->w_r, &L->xs}) want(pp, B * 4);
  want(&L->qscratch, (8 + (M + 127) / 128) * 4);
  want(&L->greedy, M * 8);
  want(&L->dheads, M * NHp * 2);
  for (int l = 0; l < NL; ++l) want(&L->dO[l], M * H * 4);
  want(&L->dc[0], (size_t)NL * B * H * 4);      // dc[l] follow dc[0]: one memset clears all
  for (int l = 0; l < NL; ++l) {
    want(&L->dG[l], (size_t)(T + 1) * B * H4 * 2);
    want(&L->hsT[l], pipe0 ? H * (B + M) * 2 : H * Mp * 2);
    want(&L->hpT[l], pipe0 ? 256 : H * Mp * 2);
    want(&L->xchg_b[l], pipe0 ? xb * 2 : 256);
  }
  want(&L->xout_b, pipe0 ? xb * 2 : 256);      // second hand-off buffer of the top layer (split placement of the fused BPTT)
  want(&L->xout_b2, pipe0 ? xb * 2 : 256);     // ... and of the lower layer (sink stage)
  want(&L->dx1, M * H * 2);
  want(&L->x1T, H * Mp * 2);
  if (nfc == 2) {
    want(&L->dx2, M * H * 2);
    want(&L->x2T, H * Mp * 2);
    want(&L->dx2T, H * Mp * 2);
  }
  want(&L->a16T, Fp * Mp * 2);
  want(&L->dGT, H4 * Mp * 2);
  want(&L->dx1T, H * Mp * 2);
  want(&L->dheadsT, NHp * Mp * 2);
  want(&L->wgrad_ws, (size_t)L->wgrad_split * H4 * std::max(H, (size_t)online->F) * 4);
  want(&L->wgrad_ws2, pipe0 ? (size_t)L->wgrad_split * H4 * H * 4 : 256);
  want(&L->heads_ws, (size_t)4 * 8 * 64 * H * 4);      // slabs of the heads' weight gradient (<= 32 K ranges x <= 64 rows x H): summed in order, no float atomics
  want(&L->dGT2, pipe0 ? H4 * Mp * 2 : 256);
  {
    // the grouped weight-gradient launch: one work item per CU -- 3/4 of them for the four LSTM problems, 1/4 for the input layer's
    const int tiles_l = 4 * (int)((H4 + 255) / 256) * (int)((H + 255) / 256), tiles_in = (int)((H + 255) / 256) * (int)((Fp + 255) / 256);
    L->group_split_l = std::max(1, std::min(8, (3 * L->n_cu / 4) / std::max(1, tiles_l)));
    L->group_split_in = std::max(1, std::min(16, (L->n_cu - tiles_l * L->group_split_l) / std::max(1, tiles_in)));
    L->group_ws_floats = pipe0 ? (int64_t)4 * (L->group_split_l + 1) * H4 * H + (int64_t)(L->group_split_in + 1) * H * Fp : 64;
    want(&L->group_ws, (size_t)L->group_ws_floats * 4);
  }
  size_t total = 0;
  for (auto& e : slots) total += e.second;
  if (L->arena.need(total + 256)) return HSAD_ERR_NOMEM;
  (void)hipMemset(L->arena.p, 0, total);
  char* p = L->arena.as<char>();
  for (auto& e : slots) {
    *e.first = p;
    p += e.second;
  }
  for (int l = 1; l < NL; ++l) L->dc[l] = L->dc[0] + (size_t)l * B * H;
  for (int q = 0; q < 2; ++q) L->xin[q] = nfc == 2 ? L->x2[q] : L->x1[q];
  return 0;
}
// optimizer state + gradient
int learner_alloc_optimizer(hsad_r2d2_learner* L) {
  const size_t np = (L->on->n_param + 3) & ~(size_t)3;      // (each of the three flat buffers 16-byte aligned)
  if (L->opt.need(np * 4 * 3 + 64)) return HSAD_ERR_NOMEM;
  (void)hipMemset(L->opt.p, 0, np * 4 * 3 + 64);
  L->gflat = L->opt.as<float>();
  L->m = L->gflat + np;
  L->v = L->m + np;
  L->osc = L->v + np;
  return 0;
}
// counter blocks (zero-initialised: a ping-pong launch clears its partner for the next one), sized for the longest chunk like the hand-off
// buffers.  Every block starts 16-byte aligned: a launch's group words at its start are 64-bit atomics, and a block of an odd word count
// (odd row blocks x odd T) misaligned the next one -- the fused forward faulted at B = 96, T = 3.
int learner_alloc_sync(hsad_r2d2_learner* L) {
  const size_t T = L->T, Tc = T, nrb = nrb_of(L->B);
  auto blk = [](size_t words) { return (words + 3) & ~(size_t)3; };
  size_t sw = 0;
  for (int k = 0; k < 2; ++k)
    for (int r = 0; r < 4; ++r) {
      L->sync_words[k][r] = (size_t)(r + 1) * nrb * (Tc + 2) + 4;
      sw += 2 * blk(L->sync_words[k][r]);
    }
  const size_t s1 = nrb * ((size_t)T + 2) + 4;
  size_t fw = 0;
  for (int k = 0; k < 3; ++k) {
    L->fsync_words[k] = ((size_t)1 << k) * nrb * ((size_t)T + 2) + 4;
    fw += 2 * blk(L->fsync_words[k]);
  }
  L->fbsync_words = (size_t)8 * nrb * ((size_t)T + 2) + 4;      // (split placement: two counter sets for the two recurrences + a projection stage)
  fw += 2 * blk(L->fbsync_words);
  if (L->sync_buf.need((sw + blk(s1) + fw) * 4)) return HSAD_ERR_NOMEM;
  (void)hipMemset(L->sync_buf.p, 0, (sw + blk(s1) + fw) * 4);
  unsigned* sp = L->sync_buf.as<unsigned>();
  for (int k = 0; k < 2; ++k)
    for (int r = 0; r < 4; ++r) {
      for (int f = 0; f < 2; ++f) {
        L->sync[k][r][f] = sp;
        sp += blk(L->sync_words[k][r]);
      }
      L->flip[k][r] = 0;
    }
  L->sync1 = sp;
  sp += blk(s1);
  for (int k = 0; k < 3; ++k)
    for (int f = 0; f < 2; ++f) {
      L->fsync[k][f] = sp;
      sp += blk(L->fsync_words[k]);
    }
  for (int f = 0; f < 2; ++f) {
    L->fbsync[f] = sp;
    sp += blk(L->fbsync_words);
  }
  return 0;
}
// the side stream, the events between the two streams and the pinned word the updates report their timeouts to
int learner_create_streams(hsad_r2d2_learner* L) {
  for (int i = 0; i < 8; ++i)
    if (hipEventCreateWithFlags(&L->ev_ck[i], learner_event_flags()) != hipSuccess) return afail(HSAD_ERR_HIP, "r2d2_learner_create: event creation failed");
  if (hipStreamCreateWithFlags(&L->side, hipStreamNonBlocking) != hipSuccess || hipEventCreateWithFlags(&L->ev_a, learner_event_flags()) != hipSuccess ||
      hipEventCreateWithFlags(&L->ev_b, learner_event_flags()) != hipSuccess || hipEventCreateWithFlags(&L->ev_c, learner_event_flags()) != hipSuccess ||
      hipEventCreateWithFlags(&L->ev_d, learner_event_flags()) != hipSuccess || hipEventCreateWithFlags(&L->ev_e, learner_event_flags()) != hipSuccess)
    return afail(HSAD_ERR_HIP, "r2d2_learner_create: stream / event creation failed");
  {
    void* hp = nullptr;      // the host word the update's timeout_gather_kernel reports to (pinned + mapped: the kernel stores into host memory)
    if (hipHostMalloc(&hp, 64, hipHostMallocMapped) == hipSuccess) {
      *(volatile unsigned*)hp = 0;
      void* dp = nullptr;
      if (hipHostGetDevicePointer(&dp, hp, 0) == hipSuccess) {
        L->h_timeout = (volatile unsigned*)hp;
        L->d_timeout = (unsigned*)dp;
      } else {
        (void)hipHostFree(hp);
      }
    }
  }
  return 0;
}

}  // namespace

extern "C" {

int hsad_r2d2_learner_create(hsad_r2d2_net* online, hsad_r2d2_net* target, int T, int rows_per_step, int multi_step, double gamma,
                             float lr, float eps, float grad_clip, hsad_r2d2_learner** out) {
  if (!online || !target || !out || T < 1 || rows_per_step < 1) return afail(HSAD_ERR_INVALID, "r2d2_learner_create: bad arguments");
  if (!online->with_backward) return afail(HSAD_ERR_INVALID, "r2d2_learner_create: the online net must be created with_backward");
  if (online->F != target->F || online->H != target->H || online->A != target->A || online->NP != target->NP || online->L != target->L ||
      online->nfc != target->nfc)
    return afail(HSAD_ERR_INVALID, "r2d2_learner_create: online / target shapes differ");
  HIP_TRY(hipSetDevice(online->device));
  auto* L = new hsad_r2d2_learner();
  L->on = online;
  L->tg = target;
  L->T = T;
  L->B = rows_per_step;
  L->M = T * rows_per_step;
  L->multi_step = multi_step;
  L->gamma = gamma;
  L->lr = lr;
  L->adam_eps = eps;
  L->clip = grad_clip;
  int dev = 0;
  (void)hipGetDevice(&dev);
  if (hipDeviceGetAttribute(&L->n_cu, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) L->n_cu = 256;
  L->Mp = pad64(L->M);
  int rc = learner_alloc_arena(L);
  if (!rc) rc = learner_alloc_optimizer(L);
  if (!rc) rc = learner_alloc_sync(L);
  if (!rc) rc = learner_create_streams(L);
  if (rc) {
    hsad_r2d2_learner_destroy(L);
    return rc;
  }
  *out = L;
  return 0;
}

void hsad_r2d2_learner_destroy(hsad_r2d2_learner* L) {
  if (!L) return;
  if (L->side) (void)hipStreamDestroy(L->side);
  for (int i = 0; i < 8; ++i)
    if (L->ev_ck[i]) (void)hipEventDestroy(L->ev_ck[i]);
  for (hipEvent_t e : {L->ev_a, L->ev_b, L->ev_c, L->ev_d, L->ev_e})
    if (e) (void)hipEventDestroy(e);
  if (L->h_timeout) (void)hipHostFree((void*)L->h_timeout);
  delete L;
}
float* hsad_r2d2_learner_grad(hsad_r2d2_learner* L) { return L ? L->gflat : nullptr; }
static int learner_reset_sync(hsad_r2d2_learner* L) {
  // the counter blocks of the ping-pong launches are laid out per launch shape: start a new schedule from clean ones
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemset(L->sync_buf.p, 0, L->sync_buf.cap));
  for (int k = 0; k < 2; ++k)
    for (int r = 0; r < 4; ++r) L->flip[k][r] = 0;
  L->fflip[0] = L->fflip[1] = L->fflip[2] = 0;
  L->fbflip = 0;
  L->fb_tc = 0;
  return 0;
}
int hsad_r2d2_learner_set_schedule(hsad_r2d2_learner* L, int chunks, int wgrad_split) {
  if (!L || chunks < 1 || wgrad_split < 1 || wgrad_split > 8) return afail(HSAD_ERR_INVALID, "learner_set_schedule: chunks >= 1, wgrad_split 1..8");
  if (chunks != L->chunks) CK(learner_reset_sync(L));
  L->chunks = chunks;
  L->wgrad_split = wgrad_split;
  return 0;
}
/* the flag word: include/hsad.h has the table.  Stored as asked for; plan_update() decides what the shape allows */
int hsad_r2d2_learner_set_fused(hsad_r2d2_learner* L, int fused_fwd) {
  if (!L) return afail(HSAD_ERR_INVALID, "null learner");
  CK(learner_reset_sync(L));
  const auto bit = [&](int b) { return (fused_fwd >> b & 1) != 0; };
  L->fused_fwd = bit(0);
  L->fused_bwd = bit(0) && !bit(1);
  L->split_refresh = bit(2);
  L->split_bptt = bit(3);
  L->proj_bptt = L->split_bptt && bit(4);
  L->sink_bptt = L->proj_bptt && bit(5);
  L->dgt_in_kernel = !bit(6);
  L->group_wgrad = !bit(7);
  const int bc = (fused_fwd >> 8) & 0xff;
  if (bc >= 1 && bc <= 8) L->bchunks = bc;
  L->btail = (fused_fwd >> 16) & 0xff;
  L->fuse_heads = !bit(24);
  L->wide_bptt = !bit(25);
  return 0;
}
// the sticky timeout words of every counter block a launch of this learner may have used (hsad_lstm_sync_timed_out semantics): a bounded
// spin that gave up leaves its word set, the kernel's outputs are then garbage
static TimeoutWords timeout_words(const hsad_r2d2_learner* L) {
  TimeoutWords w;
  w.n = 0;
  // the sticky word sits behind the counters of a launch: (recurrences) x (row blocks) x (chunk length + 2) words in
  const size_t Tc = (size_t)L->T / plan_update(L).fwd_chunks, nrb = nrb_of(L->B);
  for (int k = 0; k < 2; ++k)
    for (int r = 0; r < 4; ++r)
      for (int f = 0; f < 2; ++f) w.p[w.n++] = L->sync[k][r][f] + (size_t)(r + 1) * nrb * (Tc + 2);
  for (int k = 0; k < 3; ++k)
    for (int f = 0; f < 2; ++f) w.p[w.n++] = L->fsync[k][f] + L->fsync_words[k] - 4;
  if (L->fb_tc)
    for (int f = 0; f < 2; ++f) w.p[w.n++] = L->fbsync[f] + (size_t)L->fb_sets * nrb * (L->fb_tc + 2);
  w.p[w.n++] = L->sync1 + nrb * ((size_t)L->T + 2);      // unchunked single-recurrence launches
  return w;
}
/* synchronises and reads the words */
int hsad_r2d2_learner_timed_out(hsad_r2d2_learner* L, int32_t* timed_out) {
  if (!L || !timed_out) return afail(HSAD_ERR_INVALID, "null argument");
  HIP_TRY(hipDeviceSynchronize());
  *timed_out = 0;
  const TimeoutWords w = timeout_words(L);
  for (int i = 0; i < w.n; ++i) {
    unsigned v = 0;
    HIP_TRY(hipMemcpy(&v, w.p[i], 4, hipMemcpyDeviceToHost));
    *timed_out |= (int32_t)v;
  }
  return 0;
}
// Failing loudly where it happens: every update ends with a one-thread kernel that ORs the sticky words into a pinned
// host word; every entry point of the learner looks at that word first -- no synchronisation, so a timeout surfaces at the first call
// made after the failed update has finished on the device (at the latest one update later), whoever drives the learner.
static int timeout_gather(hsad_r2d2_learner* L, hipStream_t s) {
  if (!L->d_timeout) return 0;
  hipLaunchKernelGGL(timeout_gather_kernel, dim3(1), dim3(64), 0, s, timeout_words(L), L->d_timeout);
  HIP_TRY(hipGetLastError());
  return 0;
}
static int timeout_check(const hsad_r2d2_learner* L, const char* where) {
  if (L->h_timeout && *L->h_timeout)
    return afail(HSAD_ERR_STATE, "%s: a persistent recurrence of an earlier update gave up waiting for a sibling workgroup (were the launch's workgroups "
                                 "co-resident? foreign kernels on the device?) -- the losses, priorities and gradients since then are not valid", where);
  return 0;
}
/* test hook (fault injection): sets the sticky word of the unchunked launches' block, as a spin that gave up would */
int hsad_r2d2_learner_inject_timeout(hsad_r2d2_learner* L, int set) {
  if (!L) return afail(HSAD_ERR_INVALID, "null learner");
  HIP_TRY(hipDeviceSynchronize());
  const unsigned v = set ? 1u : 0u;
  HIP_TRY(hipMemcpy(L->sync1 + nrb_of(L->B) * ((size_t)L->T + 2), &v, 4, hipMemcpyHostToDevice));
  if (!set && L->h_timeout) *L->h_timeout = 0;
  return 0;
}

}  // extern "C"

// =====================================================================================================================
// loss forward: batch tensors [T, rows, ...] with rows = B (IQL) or B_games * num_player (VDN: Q summed over a game's players;
// reward / bootstrap [T, games], seq_len / weight / loss [games], priority [T, games]).  own_hand may be NULL (pred_weight = 0).
// =====================================================================================================================
namespace {

// the input MLP (R2D2Net.net); the online / target pair of each forward GEMM is ONE launch (hsad_gemm_nt_bf16_pair)
int fwd_input_mlp(hsad_r2d2_learner* L, const Shape& d, const float* priv_s, const void* priv_s_bf16, int n_nets, void* stream) {
  hsad_r2d2_net* nets[2] = {L->on, L->tg};
  const int M = d.M, H = d.H, Fp = d.Fp;
  // priv_s_bf16: [M, Fp] zero-padded, e.g. straight out of hsad_replay_sample (HSAD_BITS_AS_BF16); it must stay valid until
  // hsad_r2d2_loss_bwd has run (the input-layer weight gradient reads it again)
  if (priv_s_bf16) L->a16_in = (const bf16_t*)priv_s_bf16;
  else {
    CK(hsad_cast_pad_bf16(priv_s, M, d.F, d.F, L->a16, Fp, stream));
    L->a16_in = L->a16;
  }
  if (n_nets == 1) {      // the online net alone: the same GEMMs as single problems
    CK(hsad_gemm_nt_bf16(L->a16_in, Fp, nets[0]->W1, Fp, M, H, Fp, nets[0]->w(nets[0]->iB1), nullptr, 0, L->x1[0], H, 1, 0, stream));
    if (d.nfc == 2) CK(hsad_gemm_nt_bf16(L->x1[0], H, nets[0]->W2, H, M, H, H, nets[0]->w(nets[0]->iB2), nullptr, 0, L->x2[0], H, 1, 0, stream));
    return 0;
  }
  CK(hsad_gemm_nt_bf16_pair(L->a16_in, L->a16_in, Fp, nets[0]->W1, nets[1]->W1, Fp, M, H, Fp, nets[0]->w(nets[0]->iB1), nets[1]->w(nets[1]->iB1),
                            nullptr, nullptr, 0, L->x1[0], L->x1[1], H, 1, stream));
  if (d.nfc == 2)
    CK(hsad_gemm_nt_bf16_pair(L->x1[0], L->x1[1], H, nets[0]->W2, nets[1]->W2, H, M, H, H, nets[0]->w(nets[0]->iB2), nets[1]->w(nets[1]->iB2),
                              nullptr, nullptr, 0, L->x2[0], L->x2[1], H, 1, stream));
  return 0;
}

// the LSTM over the whole sequence as persistent launches with the projections computed inside the recurrences
// (hsad_lstm_forward_fused): up to two stacked layers and both nets per launch; the target net keeps neither gates nor c
int fwd_recurrence_fused(hsad_r2d2_learner* L, const Shape& d, const LearnerPlan& P, bool want_grad, int n_nets, void* stream) {
  hsad_r2d2_net* nets[2] = {L->on, L->tg};
  for (int l0 = 0; l0 < d.NL; l0 += P.fwd_layers) {
    const int g = std::min(P.fwd_layers, d.NL - l0);
    for (int q0 = 0; q0 < n_nets; q0 += P.fwd_nets) {
      hsad_lstm_fused_rec recs[4];
      for (int qi = 0; qi < P.fwd_nets; ++qi)
        for (int li = 0; li < g; ++li) {
          const int q = q0 + qi, l = l0 + li;
          hsad_lstm_fused_rec& r = recs[qi * g + li];
          r.Wih_blocked = nets[q]->Wih[l];
          r.Whh_blocked = nets[q]->Whh[l];
          r.bias_blocked = nets[q]->bg[l];
          r.x16 = li == 0 ? (l == 0 ? L->xin[q] : L->hseq[q][l - 1]) : nullptr;
          r.gates = (q == 0 && want_grad) ? L->gates[q][l] : nullptr;
          r.cseq = (q == 0 && want_grad) ? L->cseq[q][l] : nullptr;
          r.hseq16 = L->hseq[q][l];
          r.hT = L->hT[q][l];
        }
      const int nrec = P.fwd_nets * g, k = nrec == 4 ? 2 : nrec - 1;
      int& f = L->fflip[k];
      CK(hsad_lstm_forward_fused(P.fwd_nets, g, d.T, d.B, d.H, recs, L->fsync[k][f], L->fsync[k][f ^ 1], stream));
      f ^= 1;
    }
  }
  return 0;
}

// the layer-0 projection; then the layers software-pipelined over time chunks: stage st runs layer 0 on chunk st and layer 1
// on chunk st - 1, for both nets, as ONE multi-recurrence persistent launch
int fwd_recurrence_pipelined(hsad_r2d2_learner* L, const Shape& d, const LearnerPlan& P, int n_nets, void* stream) {
  hsad_r2d2_net* nets[2] = {L->on, L->tg};
  const int B = d.B, H = d.H, H4 = d.H4, nch = P.fwd_chunks;
  if (n_nets == 1)
    CK(hsad_gemm_nt_bf16(L->xin[0], H, nets[0]->Wih[0], H, d.M, H4, H, nets[0]->bg[0], L->gates[0][0], H4, nullptr, 0, 0, 0, stream));
  else
    CK(hsad_gemm_nt_bf16_pair(L->xin[0], L->xin[1], H, nets[0]->Wih[0], nets[1]->Wih[0], H, d.M, H4, H, nets[0]->bg[0], nets[1]->bg[0],
                              L->gates[0][0], L->gates[1][0], H4, nullptr, nullptr, 0, 0, stream));
  const int Tc = d.T / nch, nrb = nrb_of(B);
  const int per_launch = std::max(1, std::min(4, L->n_cu / ((H / 32) * nrb)));
  for (int st = 0; st <= nch; ++st) {
    hsad_lstm_fwd_rec recs[4];
    int nr = 0;
    for (int q = 0; q < n_nets; ++q) {
      auto rec = [&](int l, int c) {
        const size_t t0 = (size_t)c * Tc;
        hsad_lstm_fwd_rec r;
        r.gates = L->gates[q][l] + t0 * B * H4;
        r.Whh_blocked = nets[q]->Whh[l];
        r.h_prev16 = c == 0 ? L->zero16 : L->hseq[q][l] + (t0 - 1) * B * H;
        r.c_prev = c == 0 ? nullptr : L->cseq[q][l] + (t0 - 1) * B * H;
        r.hseq16 = L->hseq[q][l] + t0 * B * H;
        r.cseq = L->cseq[q][l] + t0 * B * H;
        r.hT = L->hT[q][l];
        r.xchg = L->xchg_f[q][l];
        return r;
      };
      if (st < nch) recs[nr++] = rec(0, st);
      if (st >= 1) recs[nr++] = rec(1, st - 1);
    }
    if (st >= 1) {      // layer-1 projection of chunk st - 1, both nets in one launch
      const size_t t0 = (size_t)(st - 1) * Tc;
      if (n_nets == 1)
        CK(hsad_gemm_nt_bf16(L->hseq[0][0] + t0 * B * H, H, nets[0]->Wih[1], H, Tc * B, H4, H, nets[0]->bg[1], L->gates[0][1] + t0 * B * H4, H4, nullptr,
                             0, 0, 0, stream));
      else
        CK(hsad_gemm_nt_bf16_pair(L->hseq[0][0] + t0 * B * H, L->hseq[1][0] + t0 * B * H, H, nets[0]->Wih[1], nets[1]->Wih[1], H, Tc * B, H4,
                                  H, nets[0]->bg[1], nets[1]->bg[1], L->gates[0][1] + t0 * B * H4, L->gates[1][1] + t0 * B * H4, H4, nullptr,
                                  nullptr, 0, 0, stream));
    }
    for (int i = 0; i < nr; i += per_launch) {
      const int n = std::min(per_launch, nr - i);
      int& f = L->flip[0][n - 1];
      CK(hsad_lstm_forward_chunk_multi(n, Tc, B, H, recs + i, L->sync[0][n - 1][f], L->sync[0][n - 1][f ^ 1], stream));
      f ^= 1;
    }
  }
  return 0;
}

// any T, B: per net and layer one projection GEMM + one unchunked recurrence
int fwd_recurrence_plain(hsad_r2d2_learner* L, const Shape& d, int n_nets, void* stream) {
  hsad_r2d2_net* nets[2] = {L->on, L->tg};
  for (int q = 0; q < n_nets; ++q)
    for (int l = 0; l < d.NL; ++l) {
      CK(hsad_gemm_nt_bf16(l == 0 ? L->xin[q] : L->hseq[q][l - 1], d.H, nets[q]->Wih[l], d.H, d.M, d.H4, d.H, nets[q]->bg[l], L->gates[q][l], d.H4,
                           nullptr, 0, 0, 0, stream));
      CK(hsad_lstm_layer_forward(d.T, d.B, d.H, L->gates[q][l], nets[q]->Whh[l], nullptr, L->czero, L->hseq[q][l], L->cseq[q][l], L->sc16,
                                 L->hT[q][l], L->sync1, 1, stream));
    }
  return 0;
}

// With a backward pass to follow: the transposed copies of the forward activations (operands of the weight-gradient GEMMs) start NOW on
// the side stream, next to the heads / loss chain -- once the BPTT launch holds every CU they would wait for its end
int fwd_early_transposes(hsad_r2d2_learner* L, const Shape& d, hipStream_t s) {
  void* wst = (void*)L->side;
  HIP_TRY(hipEventRecord(L->ev_e, s));
  HIP_TRY(hipStreamWaitEvent(L->side, L->ev_e, 0));
  for (int l = 0; l < d.NL; ++l) CK(transpose16(L->hseq[0][l], d.M, d.H, d.H, L->hsT[l] + d.B, d.B + d.M, nullptr, nullptr, nullptr, wst));
  CK(transpose16(L->x1[0], d.M, d.H, d.H, L->x1T, d.Mp, nullptr, nullptr, nullptr, wst));
  if (d.nfc == 2) CK(transpose16(L->x2[0], d.M, d.H, d.H, L->x2T, d.Mp, nullptr, nullptr, nullptr, wst));
  return transpose16(L->a16_in, d.M, d.Fp, d.Fp, L->a16T, d.Mp, nullptr, nullptr, nullptr, wst);
}

// IQL: heads, online Q-head and everything up to d loss / d heads.  One-launch chain: both head layers and the online dueling head are ONE
// launch, then the loss tail (which may also form d loss / d o: hd.dO_ready); four-launch chain: head GEMM pair (N = A + 1 + 3 hand columns,
// one problem alone is 80 workgroups), hsad_q_head, loss tail -- the dO GEMM follows in loss_bwd
int heads_loss_iql(hsad_r2d2_learner* L, const Shape& d, const FwdHandoff& hd, const LossArgs& b, void* stream) {
  const int M = d.M, H = d.H, NH = d.NH, A = d.A, top = d.NL - 1;
  if (hd.one_launch_heads) {
    CK(hsad_internal_heads_q(L->hseq[0][top], L->hseq[1][top], L->on->Wheads, L->tg->Wheads, L->on->bheads, L->tg->bheads, M, H, NH, A, L->heads,
                             L->heads_t, b.legal, b.a, L->q, L->qa, L->qscratch + 1, stream));
  } else {
    CK(hsad_gemm_nt_bf16_pair(L->hseq[0][top], L->hseq[1][top], H, L->on->Wheads, L->tg->Wheads, H, M, NH, H, L->on->bheads, L->tg->bheads, L->heads,
                              L->heads_t, NH, nullptr, nullptr, 0, 0, stream));
    CK(hsad_q_head(L->heads, NH, b.legal, b.a, M, A, L->q, L->qa, nullptr, L->qscratch, stream));
  }
  // (with a gradient to follow, the launch also clears d loss / d c_T of the two fused-BPTT layers: one memset less in front of the BPTT)
  return hsad_internal_loss_tail(L->heads, L->heads_t, NH, b.legal, L->q, L->qa, L->qscratch + 1, hd.one_launch_heads ? M / 128 : (M + 255) / 256, b.reward,
                                 b.bootstrap, b.seq_len, b.weight, b.own_hand, b.a, d.T, d.B, A, d.NP, L->multi_step, L->gamma, b.pred_weight, L->greedy,
                                 L->tqa, L->err, b.priority, b.loss, L->xs, b.want_grad ? L->dqa : nullptr, b.want_grad ? L->dheads : nullptr, d.NHp,
                                 hd.dc01_zero ? L->dc[0] : nullptr, hd.dc01_zero ? (int64_t)2 * d.B * H : 0, hd.dO_ready ? L->on->WheadsT : nullptr,
                                 hd.dO_ready ? L->dO[top] : nullptr, H, stream);
}

// VDN: head GEMM pair, Q-values and the double-DQN target per player, summed over a game's players, TD loss (+ the auxiliary task)
int heads_loss_vdn(hsad_r2d2_learner* L, const Shape& d, const LossArgs& b, hipStream_t s) {
  void* stream = (void*)s;
  const int T = d.T, B = d.B, M = d.M, H = d.H, NH = d.NH, A = d.A, top = d.NL - 1;
  CK(hsad_gemm_nt_bf16_pair(L->hseq[0][top], L->hseq[1][top], H, L->on->Wheads, L->tg->Wheads, H, M, NH, H, L->on->bheads, L->tg->bheads, L->heads,
                            L->heads_t, NH, nullptr, nullptr, 0, 0, stream));
  CK(hsad_q_head(L->heads, NH, b.legal, b.a, M, A, L->q, L->qa, L->greedy, L->qscratch, stream));
  CK(hsad_q_head(L->heads_t, NH, b.legal, L->greedy, M, A, L->q, L->tqa, nullptr, L->qscratch, stream));
  const float *qa = L->qa, *tqa = L->tqa;
  const int Bg = B / b.num_player;
  if (b.num_player > 1) {
    const int n = T * Bg;
    hipLaunchKernelGGL(sum_players_kernel, dim3((n + 255) / 256), dim3(256), 0, s, L->qa, n, b.num_player, L->qa_s);
    hipLaunchKernelGGL(sum_players_kernel, dim3((n + 255) / 256), dim3(256), 0, s, L->tqa, n, b.num_player, L->tqa_s);
    qa = L->qa_s;
    tqa = L->tqa_s;
  }
  CK(hsad_td_loss(qa, tqa, b.reward, b.bootstrap, b.seq_len, T, Bg, L->multi_step, L->gamma, L->err, b.priority, b.loss, b.want_grad ? L->dqa : nullptr,
                  b.weight, stream));
  if (b.pred_weight > 0) {
    CK(hsad_aux_xent(L->heads, NH, b.own_hand, T, B, A, d.NP, L->xs, stream));
    hipLaunchKernelGGL(axpy_kernel, dim3((B + 255) / 256), dim3(256), 0, s, b.loss, L->xs, b.pred_weight, B);
  }
  HIP_TRY(hipGetLastError());
  return 0;
}

int loss_fwd_impl(hsad_r2d2_learner* L, const float* priv_s, const void* priv_s_bf16, const LossArgs& b, void* stream) {
  if (!L || (!priv_s && !priv_s_bf16) || !b.legal || !b.a || !b.reward || !b.bootstrap || !b.seq_len || !b.loss || !b.priority || b.num_player < 1 ||
      L->B % b.num_player)
    return afail(HSAD_ERR_INVALID, "r2d2_loss_fwd: bad arguments");
  CK(timeout_check(L, "r2d2_loss_fwd"));
  if (b.pred_weight > 0 && b.num_player > 1)
    return afail(HSAD_ERR_INVALID, "VDN with the auxiliary task is broken in the reference (aux_task_vdn, SURVEY F6b) and has no defined behaviour");
  if (b.pred_weight > 0 && !b.own_hand) return afail(HSAD_ERR_INVALID, "r2d2_loss_fwd: pred_weight > 0 needs own_hand");
  if (b.want_grad && !b.weight) return afail(HSAD_ERR_INVALID, "r2d2_loss_fwd: the gradient needs the importance weights");
  hipStream_t s = (hipStream_t)stream;
  const Shape d = shape_of(L);
  const LearnerPlan P = plan_update(L);
  // the part of the schedule that depends on this call's arguments, and with it the whole hand-off to loss_bwd
  FwdHandoff hd;
  const bool iql = b.num_player == 1;
  hd.plan = P;
  hd.pre_T = b.want_grad && P.pipe && L->side && d.Mp == d.M;
  hd.one_launch_heads = iql && L->fuse_heads && hsad_internal_heads_q_supported(d.M, d.H, d.NH, d.A, b.legal, L->q, L->heads, L->heads_t) && d.T <= 352;
  hd.dheads_ready = iql && b.want_grad;
  hd.dO_ready = hd.one_launch_heads && b.want_grad && d.NHp == 64 && !(d.H & 31) && d.H <= (d.T <= 128 ? 512 : 256);
  hd.dc01_zero = iql && b.want_grad && d.NL >= 2;
  hd.batch = b;
  hd.have_fwd = b.want_grad;

  CK(fwd_input_mlp(L, d, priv_s, priv_s_bf16, 2, stream));
  // (the LSTM operands may still be in the side-stream half of the last optimizer step's refresh: the input layer above did not need them)
  CK(net_wait(L->on, s));
  CK(net_wait(L->tg, s));
  if (P.fwd_kind == kFused) CK(fwd_recurrence_fused(L, d, P, b.want_grad, 2, stream));
  else if (P.fwd_kind == kPipelined) CK(fwd_recurrence_pipelined(L, d, P, 2, stream));
  else CK(fwd_recurrence_plain(L, d, 2, stream));
  if (hd.pre_T) CK(fwd_early_transposes(L, d, s));
  if (iql) CK(heads_loss_iql(L, d, hd, b, stream));
  else CK(heads_loss_vdn(L, d, b, s));
  L->hand = hd;
  return 0;
}

// Behaviour cloning: the online net alone through the same stages, then the clone tail on its head outputs.  The hand-off is the one loss_bwd
// already continues from: d loss / d heads is ready, the dO GEMM and the clearing of d loss / d c_T are left to it.
// The value term of hsad_r2d2_clone_value_fwd (NULL: hsad_r2d2_clone_fwd, the policy term alone through hsad_clone_tail)
struct CloneValueTerm {
  const float* ret;
  float policy_weight, value_weight, *vloss;
  int32_t* steps;
  bool soft = false;                // hsad_r2d2_clone_soft_fwd: the cross-entropy is against `target` (hsad_clone_soft_tail)
  const float* target = nullptr;    // [T, rows, A]
};

int clone_fwd_impl(hsad_r2d2_learner* L, const float* priv_s, const void* priv_s_bf16, const LossArgs& b, int32_t* hits, int32_t* decisions, int32_t* bad,
                   const CloneValueTerm* vt, void* stream) {
  if (!L || (!priv_s && !priv_s_bf16) || !b.legal || !b.a || !b.seq_len || !b.loss || !hits || !decisions || !bad)
    return afail(HSAD_ERR_INVALID, "r2d2_clone_fwd: bad arguments");
  if (vt) {      // (what hsad_clone_value_tail would refuse, before anything is launched)
    if (!vt->steps) return afail(HSAD_ERR_INVALID, "r2d2_clone_value_fwd: bad arguments");
    if (vt->soft && !vt->target) return afail(HSAD_ERR_INVALID, "r2d2_clone_soft_fwd: no target rows (hsad_r2d2_clone_value_fwd is the call without them)");
    if (!(vt->policy_weight >= 0.f) || !(vt->value_weight >= 0.f) || std::isinf(vt->policy_weight) || std::isinf(vt->value_weight))
      return afail(HSAD_ERR_INVALID, "r2d2_clone_value_fwd: the weights of the two terms must be finite and not negative");
    if (vt->value_weight != 0.f && (!vt->ret || !vt->vloss)) return afail(HSAD_ERR_INVALID, "r2d2_clone_value_fwd: the value term needs the returns and vloss");
  }
  CK(timeout_check(L, "r2d2_clone_fwd"));
  if (b.want_grad && !b.weight) return afail(HSAD_ERR_INVALID, "r2d2_clone_fwd: the gradient needs the weights");
  hipStream_t s = (hipStream_t)stream;
  const Shape d = shape_of(L);
  const LearnerPlan P = plan_update(L, 1);
  FwdHandoff hd;
  hd.plan = P;
  hd.pre_T = b.want_grad && P.pipe && L->side && d.Mp == d.M;
  hd.dheads_ready = b.want_grad;
  hd.clone = true;
  hd.batch = b;
  hd.have_fwd = b.want_grad;

  CK(fwd_input_mlp(L, d, priv_s, priv_s_bf16, 1, stream));
  CK(net_wait(L->on, s));
  if (P.fwd_kind == kFused) CK(fwd_recurrence_fused(L, d, P, b.want_grad, 1, stream));
  else if (P.fwd_kind == kPipelined) CK(fwd_recurrence_pipelined(L, d, P, 1, stream));
  else CK(fwd_recurrence_plain(L, d, 1, stream));
  if (hd.pre_T) CK(fwd_early_transposes(L, d, s));
  const int top = d.NL - 1;
  CK(hsad_gemm_nt_bf16(L->hseq[0][top], d.H, L->on->Wheads, d.H, d.M, d.NH, d.H, L->on->bheads, L->heads, d.NH, nullptr, 0, 0, 0, stream));
  if (vt && vt->soft)
    CK(hsad_clone_soft_tail(L->heads, d.NH, b.legal, b.a, vt->target, vt->ret, b.seq_len, b.weight, d.T, d.B, d.A, vt->policy_weight, vt->value_weight, b.loss,
                            vt->vloss, hits, decisions, bad, vt->steps, b.want_grad ? L->dheads : nullptr, d.NHp, stream));
  else if (vt)
    CK(hsad_clone_value_tail(L->heads, d.NH, b.legal, b.a, vt->ret, b.seq_len, b.weight, d.T, d.B, d.A, vt->policy_weight, vt->value_weight, b.loss, vt->vloss,
                             hits, decisions, bad, vt->steps, b.want_grad ? L->dheads : nullptr, d.NHp, stream));
  else
    CK(hsad_clone_tail(L->heads, d.NH, b.legal, b.a, b.seq_len, b.weight, d.T, d.B, d.A, b.loss, hits, decisions, bad, b.want_grad ? L->dheads : nullptr,
                       d.NHp, stream));
  L->hand = hd;
  return 0;
}

}  // namespace

extern "C" int hsad_r2d2_clone_fwd(hsad_r2d2_learner* L, const float* priv_s, const void* priv_s_bf16, const float* legal_move, const int64_t* a,
                                   const float* seq_len, const float* weight, float* loss, int32_t* hits, int32_t* decisions, int32_t* bad, int want_grad,
                                   void* stream) {
  const LossArgs b{legal_move, nullptr, nullptr, seq_len, nullptr, weight, a, 1, 0.f, loss, nullptr, want_grad != 0};
  const int rc = clone_fwd_impl(L, priv_s, priv_s_bf16, b, hits, decisions, bad, nullptr, stream);
  if (rc || want_grad) return rc;       // (with a backward pass to follow, hsad_r2d2_loss_bwd gathers for both)
  return timeout_gather(L, (hipStream_t)stream);
}

extern "C" int hsad_r2d2_clone_value_fwd(hsad_r2d2_learner* L, const float* priv_s, const void* priv_s_bf16, const float* legal_move, const int64_t* a,
                                         const float* ret, const float* seq_len, const float* weight, float policy_weight, float value_weight, float* loss,
                                         float* vloss, int32_t* hits, int32_t* decisions, int32_t* bad, int32_t* steps, int want_grad, void* stream) {
  const LossArgs b{legal_move, nullptr, nullptr, seq_len, nullptr, weight, a, 1, 0.f, loss, nullptr, want_grad != 0};
  const CloneValueTerm vt{ret, policy_weight, value_weight, vloss, steps};
  const int rc = clone_fwd_impl(L, priv_s, priv_s_bf16, b, hits, decisions, bad, &vt, stream);
  if (rc || want_grad) return rc;
  return timeout_gather(L, (hipStream_t)stream);
}

extern "C" int hsad_r2d2_clone_soft_fwd(hsad_r2d2_learner* L, const float* priv_s, const void* priv_s_bf16, const float* legal_move, const int64_t* a,
                                        const float* target, const float* ret, const float* seq_len, const float* weight, float policy_weight,
                                        float value_weight, float* loss, float* vloss, int32_t* hits, int32_t* decisions, int32_t* bad, int32_t* steps,
                                        int want_grad, void* stream) {
  const LossArgs b{legal_move, nullptr, nullptr, seq_len, nullptr, weight, a, 1, 0.f, loss, nullptr, want_grad != 0};
  const CloneValueTerm vt{ret, policy_weight, value_weight, vloss, steps, true, target};
  const int rc = clone_fwd_impl(L, priv_s, priv_s_bf16, b, hits, decisions, bad, &vt, stream);
  if (rc || want_grad) return rc;
  return timeout_gather(L, (hipStream_t)stream);
}

extern "C" int hsad_r2d2_loss_fwd(hsad_r2d2_learner* L, const float* priv_s, const void* priv_s_bf16, const float* legal_move, const int64_t* a, const float* reward,
                                  const float* bootstrap, const float* seq_len, const float* own_hand, const float* weight, int num_player,
                                  float pred_weight, float* loss, float* priority, int want_grad, void* stream) {
  const LossArgs b{legal_move, reward, bootstrap, seq_len, pred_weight > 0 ? own_hand : nullptr, weight, a, num_player, pred_weight, loss, priority, want_grad != 0};
  const int rc = loss_fwd_impl(L, priv_s, priv_s_bf16, b, stream);
  if (rc || want_grad) return rc;       // (with a backward pass to follow, hsad_r2d2_loss_bwd gathers for both)
  return timeout_gather(L, (hipStream_t)stream);
}

// =====================================================================================================================
// BPTT of the last loss_fwd(want_grad = 1) of mean_b(weight_b * loss_b) into the learner's flat gradient (order = the net's
// parameter vector).  The batch tensors given to loss_fwd must still be alive.
// =====================================================================================================================
namespace {

// what every stage of a loss_bwd reads
struct BwdCtx {
  hsad_r2d2_learner* L;
  hsad_r2d2_net* on;
  Shape d;
  LearnerPlan P;
  FwdHandoff hd;
  hipStream_t s, ws;      // the caller's stream; the weight gradients' (the side stream in the pipelined schedules: they overlap the recurrences)
  void *stream, *wst;     // ... as the library's entry points take them
  float* g[kMaxP];        // the gradient of each parameter tensor
  // transposed operands.  Pipelined: [H, B + M] with x^T in columns B.., so that [:, :M] is the one-step-delayed copy (h_{t-1},
  // zeros for t = 0) and one transpose serves the input-weight and the recurrent-weight gradient.  Unchunked schedule (any T, B):
  // x^T and the delayed copy are separate zero-padded [H, Mp] buffers.
  int ldh;
  const bf16_t *hs_x[kMaxL], *hs_d[kMaxL], *xinT;
};
// what a BPTT variant leaves for the tail of the update
struct BpttLeft {
  int input_done_above = 0;      // steps >= this have their input-layer backward done on the side stream (0 = none)
  bool sink_T = false;           // d x1 transposed and the bias gradient of net.0 came out of the BPTT launch
  bool defer_l0 = false;         // layer 0's weight gradients of chunk 0 are left for the caller's stream
};

// d loss / d heads and d loss / d o of the top layer, unless the loss tail launch of loss_fwd already formed them; a clean gradient buffer
int bwd_head_gradient(const BwdCtx& c) {
  hsad_r2d2_learner* L = c.L;
  const Shape& d = c.d;
  const int P = c.hd.batch.num_player, Bg = d.B / P;
  const float *dqa = L->dqa, *weight = c.hd.batch.weight;
  if (P > 1) {
    hipLaunchKernelGGL(repeat_players_kernel, dim3((d.M + 255) / 256), dim3(256), 0, c.s, L->dqa, d.T * Bg, P, L->dqa_r);
    hipLaunchKernelGGL(repeat_players_kernel, dim3((d.B + 255) / 256), dim3(256), 0, c.s, c.hd.batch.weight, Bg, P, L->w_r);
    dqa = L->dqa_r;
    weight = L->w_r;
  }
  if (!c.hd.dheads_ready)
    CK(hsad_heads_backward(dqa, c.hd.batch.legal, c.hd.batch.a, L->heads, d.NH, c.hd.batch.own_hand, weight, d.M, d.B, d.A, d.NP, c.hd.batch.own_hand ? c.hd.batch.pred_weight / d.B : 0.f,
                           L->dheads, d.NHp, c.stream));
  if (!(c.hd.dheads_ready && c.hd.dO_ready))
    CK(hsad_gemm_nt_bf16_ex(L->dheads, d.NHp, c.on->WheadsT, d.NHp, d.M, d.H, d.NHp, nullptr, L->dO[d.NL - 1], d.H, nullptr, 0, 0, 0, 1, nullptr, 0, nullptr,
                            c.stream));
  if (!L->gflat_zero) HIP_TRY(hipMemsetAsync(L->gflat, 0, c.on->n_param * 4, c.s));
  L->gflat_zero = false;
  return 0;
}

// the transposed operands of the weight gradients (unless loss_fwd issued them already) and the heads' weight gradient, on the weight-
// gradient stream
int bwd_operands_and_heads_wgrad(const BwdCtx& c) {
  hsad_r2d2_learner* L = c.L;
  const Shape& d = c.d;
  const int B = d.B, M = d.M, Mp = d.Mp, H = d.H, NH = d.NH, NHp = d.NHp, top = d.NL - 1;
  const bool pipe = c.P.pipe;
  if (pipe) {
    HIP_TRY(hipEventRecord(L->ev_a, c.s));
    HIP_TRY(hipStreamWaitEvent(c.ws, L->ev_a, 0));
  }
  const bool pre_T = c.hd.pre_T && pipe;      // (issued by loss_fwd on the same side stream)
  for (int l = 0; l < d.NL && !pre_T; ++l) {
    // (the first B columns of the delayed copy -- h_{-1} = 0 -- are zero since the arena was created and nothing writes them)
    if (pipe) {
      CK(transpose16(L->hseq[0][l], M, H, H, L->hsT[l] + B, B + M, nullptr, nullptr, nullptr, c.wst));
    } else {
      CK(transpose16(L->hseq[0][l], M, H, H, L->hsT[l], Mp, nullptr, nullptr, nullptr, c.wst));
      if (M > B) CK(transpose16(L->hseq[0][l], M - B, H, H, L->hpT[l] + B, Mp, nullptr, nullptr, nullptr, c.wst));
    }
  }
  if (!pre_T) {
    CK(transpose16(L->x1[0], M, H, H, L->x1T, Mp, nullptr, nullptr, nullptr, c.wst));
    if (d.nfc == 2) CK(transpose16(L->x2[0], M, H, H, L->x2T, Mp, nullptr, nullptr, nullptr, c.wst));
    CK(transpose16(L->a16_in, M, d.Fp, d.Fp, L->a16T, Mp, nullptr, nullptr, nullptr, c.wst));
  }
  // the transposed operands of the input MLP (x^T, a16^T) exist: recorded BEFORE the heads' weight gradient below, which waits behind the
  // BPTT launch for a free CU -- the input-MLP chain on the caller's stream must not wait for that
  if (pipe) HIP_TRY(hipEventRecord(L->ev_d, c.ws));
  CK(transpose16(L->dheads, M, NHp, NHp, L->dheadsT, Mp, nullptr, nullptr, nullptr, c.wst));
  const int heads_split = c.P.heads_split;
  // (round 6: slabs + one ordered sum and a one-block column sum instead of float atomics -- with the BPTT launch's ticketed bias sums every
  // gradient of an update is now the same bits run to run; the chain runs on the side stream next to the BPTT launch either way)
  if (NH <= 48 && heads_split <= 32 && (H & 3) == 0 && (size_t)((M + 127) / 128) * NH <= (size_t)8 * 64 * H) {
    CK(hsad_gemm_nt_bf16_splitk_acc(L->dheadsT, Mp, c.hs_x[top], c.ldh, NH, H, Mp, heads_split, L->heads_ws, c.g[c.on->iWA], H, nullptr, c.wst));
    CK(hsad_colsum_acc_ordered(L->dheads, 1, M, NH, NHp, c.g[c.on->iBA], L->heads_ws + (size_t)3 * 8 * 64 * H, c.wst));      // (scratch: the last quarter of heads_ws; the slabs use <= 32 x 37 x H of the first three)
  } else {
    CK(hsad_gemm_nt_bf16_ex(L->dheadsT, Mp, c.hs_x[top], c.ldh, NH, H, Mp, nullptr, c.g[c.on->iWA], H, nullptr, 0, 0, 0, heads_split, nullptr, 0, nullptr, c.wst));
    CK(hsad_colsum_acc(L->dheads, 1, M, NH, NHp, c.g[c.on->iBA], nullptr, nullptr, c.wst));
  }
  // developer switch (measurement only): the BPTT launch starts behind everything issued on the side stream so far -- nothing runs next to it
  static const bool alone = getenv("HSAD_DEV_BPTT_ALONE") != nullptr;
  static hipEvent_t ev_alone = nullptr;
  if (alone && pipe) {
    if (!ev_alone) HIP_TRY(hipEventCreateWithFlags(&ev_alone, hipEventDisableTiming));
    HIP_TRY(hipEventRecord(ev_alone, c.ws));
    HIP_TRY(hipStreamWaitEvent(c.s, ev_alone, 0));
  }
  return 0;
}

// one layer's weight and bias gradients over the whole sequence (pipelined and plain BPTT), on the weight-gradient stream
int layer_wgrad(const BwdCtx& c, int l, const bf16_t* inT, int ld_in) {
  hsad_r2d2_learner* L = c.L;
  const int M = c.d.M, Mp = c.d.Mp, H = c.d.H, H4 = c.d.H4;
  float *gbi = c.g[c.on->iBih[l]], *gbh = c.g[c.on->iBhh[l]];
  if (M % 4 == 0) {      // the transpose also accumulates both bias gradients (= the un-blocked column sums of dG)
    CK(transpose16(L->dG[l], M, H4, H4, L->dGT, Mp, gbi, gbh, c.on->perm32, c.wst));
  } else {
    CK(transpose16(L->dG[l], M, H4, H4, L->dGT, Mp, nullptr, nullptr, nullptr, c.wst));
    CK(hsad_colsum_acc(L->dG[l], 1, M, H4, H4, gbi, gbh, c.on->perm32, c.wst));
  }
  CK(hsad_gemm_nt_bf16_splitk(L->dGT, Mp, inT, ld_in, H4, H, Mp, L->wgrad_split, L->wgrad_ws, c.g[c.on->iWih[l]], H, c.on->perm32, c.wst));
  return hsad_gemm_nt_bf16_splitk(L->dGT, Mp, c.hs_d[l], c.ldh, H4, H, Mp, L->wgrad_split, L->wgrad_ws, c.g[c.on->iWhh[l]], H, c.on->perm32, c.wst);
}

// fused BPTT: layer l's weight gradients of time chunk ch (contraction over its rows, added up over the chunks) on stream st
int chunk_wgrad(const BwdCtx& c, int l, int ch, void* st, bf16_t* dGT, float* wsp) {
  hsad_r2d2_learner* L = c.L;
  const int Mp = c.d.Mp, H = c.d.H, H4 = c.d.H4;
  const size_t m0 = (size_t)c.P.cut[ch] * c.d.B, Mc = (size_t)(c.P.cut[ch + 1] - c.P.cut[ch]) * c.d.B;
  if (!c.P.dgt_in_kernel)
    CK(transpose16(L->dG[l] + m0 * H4, (int)Mc, H4, H4, dGT, Mp, c.g[c.on->iBih[l]], c.g[c.on->iBhh[l]], c.on->perm32, st));
  const bf16_t* inT = l ? c.hs_x[l - 1] + m0 : c.xinT + m0;
  CK(hsad_gemm_nt_bf16_splitk_acc(dGT, Mp, inT, l ? c.ldh : Mp, H4, H, (int)Mc, L->wgrad_split, wsp, c.g[c.on->iWih[l]], H, c.on->perm32, st));
  return hsad_gemm_nt_bf16_splitk_acc(dGT, Mp, c.hs_d[l] + m0, c.ldh, H4, H, (int)Mc, L->wgrad_split, wsp, c.g[c.on->iWhh[l]], H, c.on->perm32, st);
}

// ... and the chunk's share of the input layer's backward pass (one fc layer): d x1 = dG0 W_ih0 masked by the ReLU for the chunk's rows
// (unless the sink stage wrote it), its transpose (+ bias column sums) and its contribution to dW1 (split-K atomics add up over the chunks)
int input_chunk(const BwdCtx& c, int ch, void* st) {
  hsad_r2d2_learner* L = c.L;
  const int Mp = c.d.Mp, H = c.d.H, H4 = c.d.H4, F = c.d.F;
  const size_t m0 = (size_t)c.P.cut[ch] * c.d.B, Mc = (size_t)(c.P.cut[ch + 1] - c.P.cut[ch]) * c.d.B;
  if (!c.P.use_sink)
    CK(hsad_gemm_nt_bf16_ex(L->dG[0] + m0 * H4, H4, c.on->WihT[0], H4, (int)Mc, H, H4, nullptr, nullptr, 0, L->dx1 + m0 * H, H, 0, 0, 1,
                            L->xin[0] + m0 * H, H, nullptr, st));
  CK(transpose16(L->dx1 + m0 * H, (int)Mc, H, H, L->dx1T + m0, Mp, c.g[c.on->iB1], nullptr, nullptr, st));
  return hsad_gemm_nt_bf16_ex(L->dx1T + m0, Mp, L->a16T + m0, Mp, H, F, (int)Mc, nullptr, c.g[c.on->iW1], F, nullptr, 0, 0, 0, L->wgrad_split, nullptr, 0,
                              nullptr, st);
}

// the two recurrences (k = 0: layer 1, k = 1: layer 0) of the fused BPTT launch over time chunk ch
void fused_bwd_recs(const BwdCtx& c, int ch, hsad_lstm_fused_bwd_rec recs[2]) {
  hsad_r2d2_learner* L = c.L;
  hsad_r2d2_net* on = c.on;
  const LearnerPlan& P = c.P;
  const int B = c.d.B, H = c.d.H, H4 = c.d.H4, Mp = c.d.Mp, nfc = c.d.nfc;
  const size_t t0 = (size_t)P.cut[ch];
  for (int k = 0; k < 2; ++k) {
    const int l = 1 - k;
    hsad_lstm_fused_bwd_rec& r = recs[k];
    r.WhhT_blocked = on->WhhT[l];
    r.WihT_above_blocked = k ? on->WihT[1] : nullptr;
    r.gates = L->gates[0][l] + t0 * B * H4;
    r.cseq = L->cseq[0][l] + t0 * B * H;
    r.c_before = ch == 0 ? nullptr : L->cseq[0][l] + (t0 - 1) * B * H;
    r.dO = k ? nullptr : L->dO[1] + t0 * B * H;
    r.dG16 = L->dG[l] + t0 * B * H4;
    r.dc_io = L->dc[l];
    r.has_next = ch != P.bptt_chunks - 1;
    r.xchg = L->xchg_b[l];
    r.saved_frag_major = 1;
    r.tail_is_zero = 1;
    r.xout = (P.use_split && k == 0) ? L->xout_b : nullptr;
    r.dO_stage = (P.use_proj && k == 1) ? L->dO[0] + t0 * B * H : nullptr;
    r.dGT16 = P.dgt_in_kernel ? (l == 1 ? L->dGT : L->dGT2) : nullptr;
    r.ldT = Mp;
    r.bias_grad0 = P.dgt_in_kernel ? c.g[on->iBih[l]] : nullptr;
    r.bias_grad1 = P.dgt_in_kernel ? c.g[on->iBhh[l]] : nullptr;
    r.bias_col_map = on->perm32;
    const bool snk = P.use_sink && k == 1;
    r.sink_WT = snk ? on->WihT[0] : nullptr;
    r.sink_out16 = snk ? (nfc == 2 ? L->dx2 : L->dx1) + t0 * B * H : nullptr;
    r.sink_mask16 = snk ? L->xin[0] + t0 * B * H : nullptr;
    r.sink_xout = snk ? L->xout_b2 : nullptr;
    const bool snkT = snk && P.dgt_in_kernel && nfc == 1;      // one fc layer: d x1 is only ever read transposed
    r.sink_outT16 = snkT ? L->dx1T + t0 * B : nullptr;
    r.sink_ldT = Mp;
    r.sink_bias_grad = snkT ? c.g[on->iB1] : nullptr;
    r.layout_steps = P.layout_steps;
    r.wide_blocks = P.wide_blocks ? 1 : 0;
  }
}

// Both layers of a time chunk in ONE persistent launch (hsad_lstm_backward_fused): layer 0 runs a step behind layer 1 and computes
// its dO = dG1 W_ih1 inside the recurrence.  The chunk's weight gradients run on the side stream next to the following chunk's launch.
int bptt_fused(const BwdCtx& c, BpttLeft* left) {
  hsad_r2d2_learner* L = c.L;
  const LearnerPlan& P = c.P;
  if (!c.hd.dc01_zero) HIP_TRY(hipMemsetAsync(L->dc[0], 0, (size_t)2 * c.d.B * c.d.H * 4, c.s));
  left->sink_T = P.dgt_in_kernel && c.d.nfc == 1;
  for (int ch = P.bptt_chunks - 1; ch >= 0; --ch) {
    hsad_lstm_fused_bwd_rec recs[2];
    fused_bwd_recs(c, ch, recs);
    if (L->fb_tc != P.layout_steps || L->fb_sets != P.counter_sets()) {      // another chunk length / placement: the blocks' layout changes, start from clean ones
      L->fb_sets = P.counter_sets();
      HIP_TRY(hipMemsetAsync(L->fbsync[0], 0, (size_t)(L->fbsync[1] - L->fbsync[0] + L->fbsync_words) * 4, c.s));
      L->fbflip = 0;
      L->fb_tc = P.layout_steps;
    }
    int& f = L->fbflip;
    CK(hsad_lstm_backward_fused(1, 2, P.cut[ch + 1] - P.cut[ch], c.d.B, c.d.H, recs, L->fbsync[f], L->fbsync[f ^ 1], c.stream));
    f ^= 1;
    HIP_TRY(hipEventRecord(L->ev_ck[ch], c.s));
    HIP_TRY(hipStreamWaitEvent(c.ws, L->ev_ck[ch], 0));
    if (P.group) continue;              // (one chunk: every weight gradient of the update is one grouped launch behind the BPTT)
    CK(chunk_wgrad(c, 1, ch, c.wst, L->dGT, L->wgrad_ws));
    // the last chunk's layer-0 gradients run on the caller's stream behind the input-MLP chain: two streams share the tail
    if (ch > 0) CK(chunk_wgrad(c, 0, ch, c.wst, L->dGT, L->wgrad_ws));
    else left->defer_l0 = true;
    if (P.chunk_input && ch > 0) {      // (reads x^T-side operands a16^T: behind ev_d on the same stream; writes dx1 / dx1T rows of its own)
      CK(input_chunk(c, ch, c.wst));
      left->input_done_above = P.cut[1];      // the head chunk's rows are what is left for the caller's stream
    }
  }
  return 0;
}

// rounds 1-2: stage st runs layer 1 on chunk nch - 1 - st and layer 0 (behind its stand-alone dO GEMM) on the chunk after it, as one
// multi-recurrence launch; each layer's weight gradients follow on the side stream once the layer is complete
int bptt_pipelined(const BwdCtx& c) {
  hsad_r2d2_learner* L = c.L;
  hsad_r2d2_net* on = c.on;
  const int B = c.d.B, H = c.d.H, H4 = c.d.H4, nch = c.P.fwd_chunks;
  const int Tc = c.d.T / nch, nrb = nrb_of(B);
  const size_t Mc = (size_t)Tc * B;
  if (!c.hd.dc01_zero) HIP_TRY(hipMemsetAsync(L->dc[0], 0, (size_t)2 * B * H * 4, c.s));
  const int per_launch = std::max(1, std::min(2, L->n_cu / ((H / 32) * nrb)));
  auto brec = [&](int l, int ch) {
    const size_t t0 = (size_t)ch * Tc;
    hsad_lstm_bwd_rec r;
    r.gates = L->gates[0][l] + t0 * B * H4;
    r.cseq = L->cseq[0][l] + t0 * B * H;
    r.c_before = ch == 0 ? nullptr : L->cseq[0][l] + (t0 - 1) * B * H;
    r.WhhT_blocked = on->WhhT[l];
    r.dO = L->dO[l] + t0 * B * H;
    r.dG16 = L->dG[l] + t0 * B * H4;
    r.dc_io = L->dc[l];
    r.has_next = ch != nch - 1;
    r.xchg = L->xchg_b[l];
    r.saved_frag_major = (c.P.fwd_kind == kFused) ? 1 : 0;
    r.tail_is_zero = 1;      // dG slot T: zero since the arena was created, no kernel writes it
    return r;
  };
  for (int st = 0; st <= nch; ++st) {
    hsad_lstm_bwd_rec recs[2];
    int nr = 0;
    if (st < nch) recs[nr++] = brec(1, nch - 1 - st);
    if (st >= 1) {
      const int c0 = nch - st;
      CK(hsad_gemm_nt_bf16_ex(L->dG[1] + (size_t)c0 * Mc * H4, H4, on->WihT[1], H4, (int)Mc, H, H4, nullptr, L->dO[0] + (size_t)c0 * Mc * H, H,
                              nullptr, 0, 0, 0, 1, nullptr, 0, nullptr, c.stream));
      recs[nr++] = brec(0, c0);
    }
    for (int i = 0; i < nr; i += per_launch) {
      const int n = std::min(per_launch, nr - i);
      int& f = L->flip[1][n - 1];
      CK(hsad_lstm_backward_chunk_multi(n, Tc, B, H, recs + i, L->sync[1][n - 1][f], L->sync[1][n - 1][f ^ 1], c.stream));
      f ^= 1;
    }
    if (st == nch - 1) HIP_TRY(hipEventRecord(L->ev_b, c.s));      // layer 1 complete
  }
  HIP_TRY(hipStreamWaitEvent(c.ws, L->ev_b, 0));
  CK(layer_wgrad(c, 1, c.hs_x[0], c.ldh));
  HIP_TRY(hipEventRecord(L->ev_c, c.s));                            // layer 0 complete
  HIP_TRY(hipStreamWaitEvent(c.ws, L->ev_c, 0));
  return layer_wgrad(c, 0, c.xinT, c.d.Mp);
}

// any T, B, layer count: per layer one unchunked recurrence, the dO GEMM of the layer below and the layer's weight gradients, all in line
int bptt_plain(const BwdCtx& c) {
  hsad_r2d2_learner* L = c.L;
  hsad_r2d2_net* on = c.on;
  const int T = c.d.T, B = c.d.B, M = c.d.M, H = c.d.H, H4 = c.d.H4;
  for (int l = c.d.NL - 1; l >= 0; --l) {
    if ((c.P.fwd_kind == kFused)) {      // fragment-major saved activations: one persistent launch over the whole sequence
      hsad_lstm_bwd_rec r{L->gates[0][l], L->cseq[0][l], nullptr, on->WhhT[l], L->dO[l], L->dG[l], L->dc[l], 0, nullptr, 1, 1};
      HIP_TRY(hipMemsetAsync(L->dc[l], 0, (size_t)B * H * 4, c.s));
      CK(hsad_lstm_backward_chunk_multi(1, T, B, H, &r, L->sync1, nullptr, c.stream));
    } else {
      CK(hsad_lstm_layer_backward(T, B, H, L->gates[0][l], L->cseq[0][l], nullptr, on->WhhT[l], L->dO[l], L->dG[l], L->dc[l], L->sync1, c.stream));
    }
    if (l > 0)
      CK(hsad_gemm_nt_bf16_ex(L->dG[l], H4, on->WihT[l], H4, M, H, H4, nullptr, L->dO[l - 1], H, nullptr, 0, 0, 0, 1, nullptr, 0, nullptr, c.stream));
    CK(layer_wgrad(c, l, l ? c.hs_x[l - 1] : c.xinT, l ? c.ldh : c.d.Mp));
  }
  return 0;
}

// the input MLP on the caller's stream, for the rows the BPTT left (all of them, or the head chunk's): d(last fc output) = dG_0 W_ih0 masked
// by its ReLU unless the sink stage wrote it, then one (transpose + bias column sum) per fc layer
int bwd_input_mlp(const BwdCtx& c, const BpttLeft& left, int Mi) {
  hsad_r2d2_learner* L = c.L;
  hsad_r2d2_net* on = c.on;
  const int M = c.d.M, Mp = c.d.Mp, H = c.d.H, H4 = c.d.H4, nfc = c.d.nfc;
  if (c.P.pipe) HIP_TRY(hipStreamWaitEvent(c.s, L->ev_d, 0));
  bf16_t* dxl = nfc == 2 ? L->dx2 : L->dx1;
  bf16_t* dxlT = nfc == 2 ? L->dx2T : L->dx1T;
  if (!c.P.use_sink)
    CK(hsad_gemm_nt_bf16_ex(L->dG[0], H4, on->WihT[0], H4, Mi, H, H4, nullptr, nullptr, 0, dxl, H, 0, 0, 1, L->xin[0], H, nullptr, c.stream));
  const bool fast_cs = M % 4 == 0 && H % 4 == 0;
  if (nfc == 2) {      // (always the whole batch: a chunk's share runs on the side stream with one fc layer only)
    if (fast_cs) {
      CK(transpose16(dxl, M, H, H, dxlT, Mp, c.g[on->iB2], nullptr, nullptr, c.stream));
    } else {
      CK(transpose16(dxl, M, H, H, dxlT, Mp, nullptr, nullptr, nullptr, c.stream));
      CK(hsad_colsum_acc(dxl, 1, M, H, H, c.g[on->iB2], nullptr, nullptr, c.stream));
    }
    CK(hsad_gemm_nt_bf16_ex(dxlT, Mp, L->x1T, Mp, H, H, Mp, nullptr, c.g[on->iW2], H, nullptr, 0, 0, 0, L->wgrad_split, nullptr, 0, nullptr, c.stream));
    CK(hsad_gemm_nt_bf16_ex(dxl, H, on->W2T, H, M, H, H, nullptr, nullptr, 0, L->dx1, H, 0, 0, 1, L->x1[0], H, nullptr, c.stream));
  }
  if (left.sink_T) return 0;
  if (fast_cs) return transpose16(L->dx1, Mi, H, H, L->dx1T, Mp, c.g[on->iB1], nullptr, nullptr, c.stream);
  CK(transpose16(L->dx1, Mi, H, H, L->dx1T, Mp, nullptr, nullptr, nullptr, c.stream));
  return hsad_colsum_acc(L->dx1, 1, Mi, H, H, c.g[on->iB1], nullptr, nullptr, c.stream);
}

// dW_ih1 | dW_hh1 | dW_ih0 | dW_hh0 = dG_l^T [x_l | h_l delayed]  (K = T x B, rows back in natural gate order through perm32) and
// dW_1 = dx1^T a16 -- 96 GFLOP in five problems of 8-16 tiles each: one launch, one item per CU, one slab pass (round 4: six launches
// on two streams + four slab passes, 0.22 ms)
int grouped_wgrad(const BwdCtx& c) {
  hsad_r2d2_learner* L = c.L;
  hsad_r2d2_net* on = c.on;
  const int Mp = c.d.Mp, H = c.d.H, F = c.d.F;
  hsad_gemm_group_item it[5];
  for (int k = 0; k < 4; ++k) {
    const int l = 1 - (k >> 1), hh = k & 1;
    it[k].A = l == 1 ? L->dGT : L->dGT2;
    it[k].lda = Mp;
    it[k].B = hh ? c.hs_d[l] : (l ? c.hs_x[l - 1] : c.xinT);
    it[k].ldb = (hh || l) ? c.ldh : Mp;
    it[k].C = hh ? c.g[on->iWhh[l]] : c.g[on->iWih[l]];
    it[k].ldc = H;
    it[k].row_map = on->perm32;
    it[k].M = c.d.H4; it[k].N = H; it[k].K = Mp; it[k].n_out = H;
    it[k].split_k = L->group_split_l;
    it[k].accumulate = 1;
  }
  it[4].A = L->dx1T; it[4].lda = Mp; it[4].B = L->a16T; it[4].ldb = Mp; it[4].C = c.g[on->iW1]; it[4].ldc = F; it[4].row_map = nullptr;
  it[4].M = H; it[4].N = c.d.Fp; it[4].K = Mp; it[4].n_out = F; it[4].split_k = L->group_split_in; it[4].accumulate = 1;
  if (hsad_gemm_group_workspace_floats(5, it) > L->group_ws_floats) return afail(HSAD_ERR_STATE, "loss_bwd: grouped weight-gradient workspace too small");
  return hsad_gemm_nt_bf16_group_splitk(5, it, L->group_ws, L->group_ws_floats, c.stream);
}

// the weight gradients still open on the caller's stream (one grouped launch, or net.0's and the deferred layer-0 pair), then the side
// stream joins
int bwd_weight_gradients(const BwdCtx& c, const BpttLeft& left, int Mi) {
  hsad_r2d2_learner* L = c.L;
  const int Mp = c.d.Mp, H = c.d.H, F = c.d.F;
  if (c.P.group) {
    CK(grouped_wgrad(c));
  } else {
    // (the whole batch contracts over the zero-padded length)
    CK(hsad_gemm_nt_bf16_ex(L->dx1T, Mp, L->a16T, Mp, H, F, Mi == c.d.M ? Mp : Mi, nullptr, c.g[c.on->iW1], F, nullptr, 0, 0, 0, L->wgrad_split, nullptr, 0,
                            nullptr, c.stream));
    if (left.defer_l0) CK(chunk_wgrad(c, 0, 0, c.stream, L->dGT2, L->wgrad_ws2));
  }
  if (c.P.pipe) {
    HIP_TRY(hipEventRecord(L->ev_a, c.ws));
    HIP_TRY(hipStreamWaitEvent(c.s, L->ev_a, 0));
  }
  return 0;
}

int loss_bwd_impl(hsad_r2d2_learner* L, void* stream) {
  if (L) CK(net_wait(L->on, (hipStream_t)stream));
  if (!L || !L->hand.have_fwd) return afail(HSAD_ERR_STATE, "r2d2_loss_bwd: call loss_fwd(want_grad = 1) first");
  CK(timeout_check(L, "r2d2_loss_bwd"));
  L->hand.have_fwd = false;
  plan_bptt(L, L->hand.plan);      // (the backward flags may have changed since loss_fwd; the forward that ran has not)
  BwdCtx c;
  c.L = L;
  c.on = L->on;
  c.d = shape_of(L);
  c.P = L->hand.plan;
  c.hd = L->hand;
  const bool pipe = c.P.pipe;
  c.s = (hipStream_t)stream;
  c.ws = pipe ? L->side : c.s;
  c.stream = stream;
  c.wst = (void*)c.ws;
  for (int i = 0; i < c.on->np; ++i) c.g[i] = L->gflat + c.on->off[i];
  c.ldh = pipe ? c.d.B + c.d.M : c.d.Mp;            // (Mp == M in the pipelined schedules)
  for (int l = 0; l < c.d.NL; ++l) {
    c.hs_x[l] = pipe ? L->hsT[l] + c.d.B : L->hsT[l];
    c.hs_d[l] = pipe ? L->hsT[l] : L->hpT[l];
  }
  c.xinT = c.d.nfc == 2 ? L->x2T : L->x1T;
  CK(bwd_head_gradient(c));
  CK(bwd_operands_and_heads_wgrad(c));
  BpttLeft left;
  if (c.P.bwd_kind == kFused) CK(bptt_fused(c, &left));
  else if (c.P.bwd_kind == kPipelined) CK(bptt_pipelined(c));
  else CK(bptt_plain(c));
  const int Mi = left.input_done_above ? left.input_done_above * c.d.B : c.d.M;      // rows of the input layer still to do
  CK(bwd_input_mlp(c, left, Mi));
  return bwd_weight_gradients(c, left, Mi);
}

}  // namespace

extern "C" {

/* loss_bwd with importance weights that were not known at loss_fwd time: torch.autograd hands d objective / d loss_b to the backward of
 * R2D2Agent.loss (the reference driver forms (loss * weight).mean() AFTER agent.loss returned: pyhanabi/selfplay.py:226-228), i.e.
 * weight_b = B * d objective / d loss_b.  Recomputes d loss / d qa from the saved TD errors and lets loss_bwd rebuild d loss / d heads
 * (the un-fused heads-backward kernel: the same arithmetic as the fused loss tail).  weight, seq_len: [games], alive until the call returns
 * its work to the stream. */
int hsad_r2d2_loss_bwd_weighted(hsad_r2d2_learner* L, const float* weight, const float* seq_len, void* stream) {
  if (!L || !weight || !seq_len) return afail(HSAD_ERR_INVALID, "r2d2_loss_bwd_weighted: null argument");
  if (!L->hand.have_fwd) return afail(HSAD_ERR_STATE, "r2d2_loss_bwd: call loss_fwd(want_grad = 1) first");
  if (L->hand.clone)
    return afail(HSAD_ERR_STATE, "r2d2_loss_bwd_weighted: the last forward was hsad_r2d2_clone_fwd -- it keeps no TD errors to re-weight; give the weights "
                                 "to clone_fwd and call hsad_r2d2_loss_bwd");
  const int Bg = L->B / L->hand.batch.num_player, n = L->T * Bg;
  hipLaunchKernelGGL(dqa_reweight_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, L->err, seq_len, weight, L->T, Bg, L->dqa);
  HIP_TRY(hipGetLastError());
  L->hand.batch.weight = weight;
  L->hand.dheads_ready = false;
  return hsad_r2d2_loss_bwd(L, stream);
}

/* learning rate, Adam epsilon and the clipping norm of hsad_r2d2_optimizer_step (<= 0: no clipping), changeable between steps */
int hsad_r2d2_learner_set_optim(hsad_r2d2_learner* L, float lr, float eps, float max_grad_norm) {
  if (!L || !(lr >= 0.f) || !(eps > 0.f)) return afail(HSAD_ERR_INVALID, "r2d2_learner_set_optim: bad argument");
  L->lr = lr;
  L->adam_eps = eps;
  L->clip = max_grad_norm > 0.f ? max_grad_norm : 3.0e38f;
  return 0;
}

int hsad_r2d2_loss_bwd(hsad_r2d2_learner* L, void* stream) {
  const int rc = loss_bwd_impl(L, stream);
  return rc ? rc : timeout_gather(L, (hipStream_t)stream);      // the update's persistent launches are all enqueued: collect their sticky words behind them
}

/* what the last loss_fwd ran and -- as the loss_bwd behind it resolved it, else as it would be under the current flags -- its backward half */
int hsad_r2d2_learner_plan(const hsad_r2d2_learner* L, hsad_learner_plan* out) {
  if (!L || !out) return afail(HSAD_ERR_INVALID, "r2d2_learner_plan: null argument");
  if (L->hand.plan.fwd_kind < 0) return afail(HSAD_ERR_STATE, "r2d2_learner_plan: call loss_fwd first");
  const LearnerPlan& P = L->hand.plan;
  *out = {P.fwd_kind, P.fwd_nets, P.fwd_layers, P.fwd_chunks, P.bwd_kind, P.bptt_chunks, P.use_split, P.use_proj, P.use_sink, P.dgt_in_kernel,
          P.group, P.wide_blocks, P.chunk_input, L->hand.one_launch_heads, L->hand.dO_ready};
  return 0;
}

// torch.nn.utils.clip_grad_norm_ + Adam.step (selfplay.py:231-235) on the online net + re-derivation of its kernel operands.
// grad_norm_sq_dev (may be NULL): device float that receives the squared pre-clip global gradient norm.
int hsad_r2d2_optimizer_step(hsad_r2d2_learner* L, float beta1, float beta2, float** grad_norm_sq_dev, void* stream) {
  if (!L) return afail(HSAD_ERR_INVALID, "null learner");
  CK(timeout_check(L, "r2d2_optimizer_step"));
  L->step_count++;
  float* slot = nullptr;
  CK(hsad_adam_step_zero_grad(L->on->flat, L->gflat, L->m, L->v, (int64_t)L->on->n_param, L->clip, L->lr, beta1, beta2, L->adam_eps, L->step_count,
                              L->osc, &slot, stream));
  L->gflat_zero = true;
  if (grad_norm_sq_dev) *grad_norm_sq_dev = slot;
  if (L->side && L->split_refresh) return net_refresh_split(L->on, (hipStream_t)stream, L->side, L->ev_b);
  return net_refresh(L->on, (hipStream_t)stream);
}

const float* hsad_r2d2_learner_grad_norm_dev(const hsad_r2d2_learner* L) { return L ? L->osc + 4 + L->step_count % 12 : nullptr; }

int hsad_r2d2_sync_target_with_online(hsad_r2d2_learner* L, void* stream) {
  if (!L) return afail(HSAD_ERR_INVALID, "null learner");
  HIP_TRY(hipMemcpyAsync(L->tg->flat, L->on->flat, L->on->n_param * 4, hipMemcpyDeviceToDevice, (hipStream_t)stream));
  return net_refresh(L->tg, (hipStream_t)stream);
}

}  // extern "C"
