// hsad_agent.hip — the COMPOSITE entry points of the drop-in boundary (include/hsad.h: hsad_r2d2_net_*, hsad_r2d2_act, hsad_r2d2_q_of,
// hsad_r2d2_compute_priority); the learner (hsad_r2d2_learner_*, hsad_r2d2_loss_fwd / _loss_bwd / _optimizer_step) is csrc/hsad_learner.hip.
//
// What they replace: the methods the reference's native side calls on the agent -- `act` and `compute_priority` through
// rela::BatchRunner (rela/batch_runner.h:74-113, rela/r2d2_actor.h:61-172 -> pyhanabi/r2d2.py:247-361) -- and the learner step
// of pyhanabi/selfplay.py:208-244 (R2D2Agent.loss, r2d2.py:383-499; backward; clip; Adam).  A C++ / pybind host can run the
// agent and the learner through these calls alone: the whole kernel schedule (operand casts, GEMMs, fused cells, persistent
// recurrences pipelined over layers and time chunks, heads, TD loss, BPTT, weight gradients on a side stream, Adam, operand
// refresh) lives here, behind plain pointers.  The library owns the weights (one flat fp32 vector per net, tensors in the
// order of hsad_r2d2_param_name), every bf16 operand copy and all workspace; callers own inputs and outputs.
//
// The kernels themselves are the ones in hsad_r2d2.hip, reached through their C entry points.
#include <algorithm>
#include <vector>

#include "hsad_agent_internal.h"

namespace {

size_t net_tensor_elems(const hsad_r2d2_net* n, int i) {
  const size_t H = n->H, F = n->F, A = n->A, NP = n->NP;
  if (i == n->iW1) return H * F;
  if (i == n->iB1 || i == n->iB2 || i == n->iWV) return H;
  if (i == n->iW2) return H * H;
  for (int l = 0; l < n->L; ++l) {
    if (i == n->iWih[l] || i == n->iWhh[l]) return 4 * H * H;
    if (i == n->iBih[l] || i == n->iBhh[l]) return 4 * H;
  }
  if (i == n->iWA) return A * H;
  if (i == n->iWP) return NP * H;
  if (i == n->iBA) return A;
  if (i == n->iBV) return 1;
  return NP;
}

void net_build_table(hsad_r2d2_net* n) {
  int k = 0;
  auto add = [&](const std::string& nm) {
    n->names[k] = nm;
    return k++;
  };
  n->iW1 = add("net.0.weight");
  n->iB1 = add("net.0.bias");
  if (n->nfc == 2) {
    n->iW2 = add("net.2.weight");
    n->iB2 = add("net.2.bias");
  }
  for (int l = 0; l < n->L; ++l) {
    const std::string sfx = "_l" + std::to_string(l);
    n->iWih[l] = add("lstm.weight_ih" + sfx);
    n->iWhh[l] = add("lstm.weight_hh" + sfx);
    n->iBih[l] = add("lstm.bias_ih" + sfx);
    n->iBhh[l] = add("lstm.bias_hh" + sfx);
  }
  n->iWA = add("fc_a.weight");
  n->iWV = add("fc_v.weight");
  n->iWP = add("pred.weight");
  n->iBA = add("fc_a.bias");
  n->iBV = add("fc_v.bias");
  n->iBP = add("pred.bias");
  n->np = k;
}

// part: 1 = the input MLP, the heads and every bias (small), 2 = the LSTM weight matrices (forward and transposed layouts), 3 = both
int net_refresh_part(hsad_r2d2_net* n, hipStream_t s, int part) {
  const int H = n->H;
  // every derived operand in one launch: weight jobs first, then the biases
  CK(hsad_refresh_begin());
  if (part & 1) {
    CK(hsad_refresh_add_weight(n->w(n->iW1), H, n->F, n->F, nullptr, n->W1, n->Fp, nullptr, 0));
    if (n->nfc == 2) CK(hsad_refresh_add_weight(n->w(n->iW2), H, H, H, nullptr, n->W2, H, n->with_backward ? n->W2T : nullptr, H));
  }
  if (part & 2)
    for (int l = 0; l < n->L; ++l) {
      const float* wih = n->w(n->iWih[l]);
      const float* whh = n->w(n->iWhh[l]);
      CK(hsad_refresh_add_weight(wih, 4 * H, H, H, n->perm32, n->Wih[l], H, n->with_backward ? n->WihT[l] : nullptr, 4 * H));
      CK(hsad_refresh_add_weight(whh, 4 * H, H, H, n->perm32, n->Whh[l], H, n->with_backward ? n->WhhT[l] : nullptr, 4 * H));
      if (n->Wcat16[l] && !n->with_backward) {
        CK(hsad_refresh_add_weight(wih, 4 * H, H, H, n->perm16, n->Wcat16[l], 2 * H, nullptr, 0));
        CK(hsad_refresh_add_weight(whh, 4 * H, H, H, n->perm16, n->Wcat16[l] + H, 2 * H, nullptr, 0));
      }
    }
  if (part & 1) {
    const int wi[3] = {n->iWA, n->iWV, n->iWP}, bi[3] = {n->iBA, n->iBV, n->iBP}, rows[3] = {n->A, 1, n->NP};
    int r0 = 0;
    for (int k = 0; k < 3; ++k) {
      CK(hsad_refresh_add_weight(n->w(wi[k]), rows[k], H, H, nullptr, n->Wheads + (size_t)r0 * H, H,
                                 n->with_backward ? n->WheadsT + r0 : nullptr, n->NHp));
      r0 += rows[k];
    }
    for (int l = 0; l < n->L; ++l) {
      const float* bih = n->w(n->iBih[l]);
      const float* bhh = n->w(n->iBhh[l]);
      CK(hsad_refresh_add_bias(bih, bhh, n->perm32, n->bg[l], 4 * H));
      if (n->Wcat16[l] && !n->with_backward) CK(hsad_refresh_add_bias(bih, bhh, n->perm16, n->bias16[l], 4 * H));
    }
    r0 = 0;
    for (int k = 0; k < 3; ++k) {
      CK(hsad_refresh_add_bias(n->w(bi[k]), nullptr, nullptr, n->bheads + r0, rows[k]));
      r0 += rows[k];
    }
  }
  CK(hsad_refresh_launch((void*)s));
  return 0;
}

__global__ void add_bf16_kernel(const bf16_t* __restrict__ a, const bf16_t* __restrict__ b, bf16_t* __restrict__ out, size_t n) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float s = __uint_as_float((uint32_t)a[i] << 16) + __uint_as_float((uint32_t)b[i] << 16);
  uint32_t u = __float_as_uint(s);
  u += 0x7fffu + ((u >> 16) & 1u);
  out[i] = (bf16_t)(u >> 16);
}

// the input MLP (R2D2Net.net: Linear + ReLU, x num_fc_layer) on N rows: a16 [N, Fp] -> x [N, H] bf16.  tmp: [N, H] bf16 scratch (2 layers)
int net_input_mlp(hsad_r2d2_net* n, int N, const bf16_t* a16, bf16_t* x, bf16_t* tmp, void* st) {
  const int H = n->H;
  if (n->nfc == 1) return hsad_gemm_nt_bf16(a16, n->Fp, n->W1, n->Fp, N, H, n->Fp, n->w(n->iB1), nullptr, 0, x, H, 1, 0, st);
  CK(hsad_gemm_nt_bf16(a16, n->Fp, n->W1, n->Fp, N, H, n->Fp, n->w(n->iB1), nullptr, 0, tmp, H, 1, 0, st));
  return hsad_gemm_nt_bf16(tmp, H, n->W2, H, N, H, H, n->w(n->iB2), nullptr, 0, x, H, 1, 0, st);
}

// fp32 [L*N, H] -> bf16 scratch, x-projection etc.: the single-step trunk (R2D2Net.act, r2d2.py:65-78) on N rows.
// out: o16 = lstm output bf16 [N,H] (points into ws), optional new state.  h16_in: bf16(h0) [L,N,H] when the caller has it.
// with_skip: o16 = lstm output + x (skip_connect applies in R2D2Net.act only, r2d2.py:74-75; forward() ignores it)
struct StepOut {
  bf16_t* o16;
  bf16_t* h16_new;   // [L,N,H] (fused path only, else null)
};

int net_step(hsad_r2d2_net* n, int N, const bf16_t* a16, const float* h0, const float* c0, const bf16_t* h16_in, float* h_out,
             float* c_out, char* wsp, StepOut* out, hipStream_t s, bf16_t* h16_dst = nullptr, bool x_ready = false, bool with_skip = false) {
  const int H = n->H, L = n->L;
  void* st = (void*)s;
  const size_t NH_ = (size_t)N * H;
  bf16_t* x = reinterpret_cast<bf16_t*>(wsp);   // x_ready: the caller already ran the input layer into the head of wsp
  wsp += NH_ * 2;
  bf16_t* xtmp = reinterpret_cast<bf16_t*>(wsp);  // second fc layer / skip sum
  wsp += NH_ * 2;
  if (!x_ready) CK(net_input_mlp(n, N, a16, x, xtmp, st));
  const bool fused = n->Wcat16[0] && !n->with_backward && N >= 1024;
  bf16_t* o16 = nullptr;
  if (fused) {
    bf16_t* h16 = reinterpret_cast<bf16_t*>(wsp);
    wsp += L * NH_ * 2;
    bf16_t* h16n = h16_dst ? h16_dst : reinterpret_cast<bf16_t*>(wsp);   // h16_dst: the caller's [L,N,H] buffer, written in place
    wsp += L * NH_ * 2;
    if (!h16_in) {
      CK(hsad_cast_pad_bf16(h0, L * N, H, H, h16, H, st));
      h16_in = h16;
    }
    const bf16_t* xin = x;
    for (int l = 0; l < L; ++l) {
      CK(hsad_lstm_cell_fused(N, H, H, xin, H, h16_in + (size_t)l * NH_, n->Wcat16[l], n->bias16[l], c0 + (size_t)l * NH_,
                              c_out ? c_out + (size_t)l * NH_ : nullptr, h_out ? h_out + (size_t)l * NH_ : nullptr,
                              h16n + (size_t)l * NH_, st));
      xin = h16n + (size_t)l * NH_;
    }
    o16 = h16n + (size_t)(L - 1) * NH_;
    out->h16_new = h16n;
  } else {
    // small batches: projection GEMM + one recurrence step per layer
    float* gates = reinterpret_cast<float*>(wsp);
    wsp += (size_t)N * 4 * H * 4;
    bf16_t* hseq = reinterpret_cast<bf16_t*>(wsp);
    wsp += L * NH_ * 2;
    bf16_t* sc16 = reinterpret_cast<bf16_t*>(wsp);
    wsp += NH_ * 2;
    float* cs = reinterpret_cast<float*>(wsp);
    wsp += L * NH_ * 4;
    float* ht = reinterpret_cast<float*>(wsp);
    wsp += L * NH_ * 4;
    const bf16_t* inp = x;
    for (int l = 0; l < L; ++l) {
      CK(hsad_gemm_nt_bf16(inp, H, n->Wih[l], H, N, 4 * H, H, n->bg[l], gates, 4 * H, nullptr, 0, 0, 0, st));
      CK(hsad_lstm_layer_forward(1, N, H, gates, n->Whh[l], h0 + (size_t)l * NH_, c0 + (size_t)l * NH_, hseq + (size_t)l * NH_,
                                 c_out ? c_out + (size_t)l * NH_ : cs + (size_t)l * NH_, sc16,
                                 h_out ? h_out + (size_t)l * NH_ : ht + (size_t)l * NH_, nullptr, 0, st));
      inp = hseq + (size_t)l * NH_;
    }
    o16 = hseq + (size_t)(L - 1) * NH_;
    out->h16_new = nullptr;
  }
  if (with_skip && n->skip) {
    hipLaunchKernelGGL(add_bf16_kernel, dim3((unsigned)((NH_ + 255) / 256)), dim3(256), 0, s, o16, x, xtmp, NH_);
    HIP_TRY(hipGetLastError());
    o16 = xtmp;
  }
  out->o16 = o16;
  return 0;
}

// The trunks of the online and the target net of an acting step, layer by layer as ONE launch of two cell problems
// (hsad_lstm_cell_fused_pair): input layers already in the heads of the two workspaces, both nets on the fused inference path, same
// shape, no skip connection.  Workspace layout and results as two net_step calls (the target reads the online pass's bf16 state).
int net_step_pair(hsad_r2d2_net* n, hsad_r2d2_net* tg, int N, const float* h0, const float* c0, const bf16_t* h16_in, float* h_out, float* c_out,
                  char* ws_on, char* ws_tg, StepOut* so, StepOut* st, hipStream_t s, bf16_t* h16_dst) {
  const int H = n->H, L = n->L;
  void* stp = (void*)s;
  const size_t NH_ = (size_t)N * H;
  bf16_t* x_on = reinterpret_cast<bf16_t*>(ws_on);
  bf16_t* x_tg = reinterpret_cast<bf16_t*>(ws_tg);
  bf16_t* h16 = reinterpret_cast<bf16_t*>(ws_on + 2 * NH_ * 2);
  bf16_t* h16n_on = h16_dst ? h16_dst : reinterpret_cast<bf16_t*>(ws_on + 2 * NH_ * 2 + L * NH_ * 2);
  bf16_t* h16n_tg = reinterpret_cast<bf16_t*>(ws_tg + 2 * NH_ * 2 + L * NH_ * 2);
  if (!h16_in) {
    CK(hsad_cast_pad_bf16(h0, L * N, H, H, h16, H, stp));
    h16_in = h16;
  }
  const bf16_t *xin_on = x_on, *xin_tg = x_tg;
  for (int l = 0; l < L; ++l) {
    CK(hsad_lstm_cell_fused_pair(N, H, H, H, xin_on, xin_tg, h16_in + (size_t)l * NH_, h16_in + (size_t)l * NH_, n->Wcat16[l], tg->Wcat16[l], n->bias16[l],
                                 tg->bias16[l], c0 + (size_t)l * NH_, c0 + (size_t)l * NH_, c_out ? c_out + (size_t)l * NH_ : nullptr, nullptr,
                                 h_out ? h_out + (size_t)l * NH_ : nullptr, nullptr, h16n_on + (size_t)l * NH_, h16n_tg + (size_t)l * NH_, stp));
    xin_on = h16n_on + (size_t)l * NH_;
    xin_tg = h16n_tg + (size_t)l * NH_;
  }
  so->o16 = h16n_on + (size_t)(L - 1) * NH_;
  so->h16_new = h16n_on;
  st->o16 = h16n_tg + (size_t)(L - 1) * NH_;
  st->h16_new = h16n_tg;
  return 0;
}

size_t step_ws_bytes(const hsad_r2d2_net* n, int N) {
  const size_t NH_ = (size_t)N * n->H, L = n->L;
  return 2 * NH_ * 2 + std::max<size_t>(2 * L * NH_ * 2, (size_t)N * 4 * n->H * 4 + (L + 1) * NH_ * 2 + 2 * L * NH_ * 4) + 256;
}

// the workspace of a network pass on N rows, carved from n->ws: a16 | `nets` step areas | `nets` heads | scratch | extra
struct PassWs {
  bf16_t* a16;     // [N, Fp] the observation in bf16 (obs_bf16 points it at the caller's copy when there is one)
  char* step[2];   // net_step's / net_step_pair's workspaces
  float* hd[2];    // [N, NH] heads
  float* scratch;  // the acting tail's block minima
  char* extra;     // extra_b bytes, 16-byte aligned
};

int pass_ws(hsad_r2d2_net* n, int N, int nets, size_t extra_b, PassWs* w) {
  const size_t a16_b = (size_t)N * n->Fp * 2, hd_b = (size_t)N * n->NH * 4, sc_b = (4 + (N + 255) / 256) * 4, step_b = step_ws_bytes(n, N);
  CK(n->ws.need(a16_b + nets * (step_b + hd_b) + sc_b + 1024 + extra_b));
  char* p = n->ws.as<char>();
  w->a16 = (bf16_t*)p;
  p += a16_b;
  for (int k = 0; k < nets; ++k, p += step_b) w->step[k] = p;
  for (int k = 0; k < nets; ++k, p += hd_b) w->hd[k] = (float*)p;
  w->scratch = (float*)p;
  w->extra = (char*)(((uintptr_t)p + sc_b + 15) & ~(uintptr_t)15);
  return 0;
}

// the observation as the GEMMs read it: priv_s_bf16 ([N, Fp] as hsad_env_bind_packed writes it) adopted, else priv_s cast into w->a16
int obs_bf16(hsad_r2d2_net* n, int N, const float* priv_s, const void* priv_s_bf16, PassWs* w, void* stream) {
  if (priv_s_bf16) w->a16 = (bf16_t*)priv_s_bf16;
  else CK(hsad_cast_pad_bf16(priv_s, N, n->F, n->F, w->a16, n->Fp, stream));
  return 0;
}

// one net from the observation to its heads in w->hd[k]: obs_bf16, net_step in w->step[k] (arguments as net_step's), the heads GEMM
int net_heads(hsad_r2d2_net* n, int N, const float* priv_s, const void* priv_s_bf16, const float* h0, const float* c0, const bf16_t* h16_in,
              float* h_out, float* c_out, PassWs* w, int k, StepOut* so, hipStream_t s, bf16_t* h16_dst = nullptr, bool x_ready = false,
              bool with_skip = false) {
  CK(obs_bf16(n, N, priv_s, priv_s_bf16, w, (void*)s));
  CK(net_step(n, N, w->a16, h0, c0, h16_in, h_out, c_out, w->step[k], so, s, h16_dst, x_ready, with_skip));
  return hsad_gemm_nt_bf16(so->o16, n->H, n->Wheads, n->H, N, n->NH, n->H, n->bheads, w->hd[k], n->NH, nullptr, 0, 0, 0, (void*)s);
}

}  // namespace

// a stream about to read the net's LSTM operands: behind the side-stream half of the last split refresh
int net_wait(hsad_r2d2_net* n, hipStream_t s) {
  if (n->split_pending && hipStreamWaitEvent(s, n->ev_refresh, 0) != hipSuccess) return afail(HSAD_ERR_HIP, "hipStreamWaitEvent(refresh) failed");
  return 0;
}

int net_refresh(hsad_r2d2_net* n, hipStream_t s) {
  CK(net_wait(n, s));          // (the pending half writes the same buffers)
  n->version++;
  return net_refresh_part(n, s, 3);
}

// the same with the big half (LSTM matrices, ~95 % of the bytes) on `side`, ordered behind everything enqueued on `s` so far; `s` only
// carries the small half, so the next update's input layer starts ~13 us earlier and the LSTM half runs next to it
int net_refresh_split(hsad_r2d2_net* n, hipStream_t s, hipStream_t side, hipEvent_t ev_tmp) {
  CK(net_wait(n, s));
  if (!n->ev_refresh && hipEventCreateWithFlags(&n->ev_refresh, hipEventDisableTiming) != hipSuccess) return afail(HSAD_ERR_HIP, "hipEventCreate failed");
  n->version++;
  HIP_TRY(hipEventRecord(ev_tmp, s));
  HIP_TRY(hipStreamWaitEvent(side, ev_tmp, 0));
  CK(net_refresh_part(n, side, 2));
  HIP_TRY(hipEventRecord(n->ev_refresh, side));
  n->split_pending = true;
  return net_refresh_part(n, s, 1);
}

extern "C" {

/* the default architecture's table (16 tensors); nets created with hsad_r2d2_net_create_ex report theirs through the _net_ variants */
int hsad_r2d2_num_params(void) { return 16; }
const char* hsad_r2d2_param_name(int i) {
  static const char* kDefault[16] = {"net.0.weight",      "net.0.bias",        "lstm.weight_ih_l0", "lstm.weight_hh_l0",
                                     "lstm.bias_ih_l0",   "lstm.bias_hh_l0",   "lstm.weight_ih_l1", "lstm.weight_hh_l1",
                                     "lstm.bias_ih_l1",   "lstm.bias_hh_l1",   "fc_a.weight",       "fc_v.weight",
                                     "pred.weight",       "fc_a.bias",         "fc_v.bias",         "pred.bias"};
  return (i >= 0 && i < 16) ? kDefault[i] : nullptr;
}
int hsad_r2d2_net_num_params(const hsad_r2d2_net* n) { return n ? n->np : 0; }
const char* hsad_r2d2_net_param_name(const hsad_r2d2_net* n, int i) { return (n && i >= 0 && i < n->np) ? n->names[i].c_str() : nullptr; }
int hsad_r2d2_net_arch(const hsad_r2d2_net* n, int32_t* num_fc_layer, int32_t* num_lstm_layer, int32_t* skip_connect) {
  if (!n) return afail(HSAD_ERR_INVALID, "null net");
  if (num_fc_layer) *num_fc_layer = n->nfc;
  if (num_lstm_layer) *num_lstm_layer = n->L;
  if (skip_connect) *skip_connect = n->skip ? 1 : 0;
  return 0;
}

// (hsad_actor_partner.inc: what a frozen network partner is held against, and the shape of its carried state)
int hsad_internal_net_dims(const hsad_r2d2_net* n, int* in_dim, int* hid_dim, int* num_action, int* num_lstm_layer, int* device) {
  if (!n) return afail(HSAD_ERR_INVALID, "null net");
  *in_dim = n->F;
  *hid_dim = n->H;
  *num_action = n->A;
  *num_lstm_layer = n->L;
  *device = n->device;
  return 0;
}

int hsad_r2d2_net_create_ex(int in_dim, int hid_dim, int num_action, int hand_size, int num_fc_layer, int num_lstm_layer, int skip_connect,
                            int with_backward, int device, hsad_r2d2_net** out) {
  if (!out || in_dim < 1 || num_action < 1 || hand_size < 1) return afail(HSAD_ERR_INVALID, "r2d2_net_create: bad dimensions");
  if (hid_dim < 64 || hid_dim % 64) return afail(HSAD_ERR_INVALID, "r2d2_net_create: hid_dim must be a multiple of 64");
  if (num_fc_layer < 1 || num_fc_layer > 2) return afail(HSAD_ERR_INVALID, "r2d2_net_create: num_fc_layer must be 1 or 2");
  if (num_lstm_layer < 1 || num_lstm_layer > kMaxL) return afail(HSAD_ERR_INVALID, "r2d2_net_create: num_lstm_layer must be 1..%d", kMaxL);
  HIP_TRY(hipSetDevice(device));
  auto* n = new hsad_r2d2_net();
  n->F = in_dim;
  n->Fp = pad64(in_dim);
  n->H = hid_dim;
  n->A = num_action;
  n->NP = 3 * hand_size;
  n->NH = n->A + 1 + n->NP;
  n->NHp = pad64(n->NH);
  n->device = device;
  n->nfc = num_fc_layer;
  n->L = num_lstm_layer;
  n->skip = skip_connect != 0;
  n->with_backward = with_backward != 0;
  net_build_table(n);
  size_t o = 0;
  for (int i = 0; i < n->np; ++i) {
    n->off[i] = o;
    o += net_tensor_elems(n, i);     // back to back: [fc_a | fc_v | pred] weights / biases form contiguous [NH, H] / [NH] blocks
  }
  n->off[n->np] = o;
  n->n_param = o;
  if (n->flat_buf.need(o * 4)) {
    delete n;
    return HSAD_ERR_NOMEM;
  }
  n->flat = n->flat_buf.as<float>();
  (void)hipMemset(n->flat, 0, o * 4);
  const size_t H = hid_dim, H4 = 4 * H, L = n->L;
  // operand arena
  size_t need = H * n->Fp * 2 + 2 * H * H * 2 + L * (H4 * H * 2) * 2 + L * H4 * 4 + (size_t)n->NH * H * 2 + n->NHp * 4 + L * (H4 * 2 * H * 2) + L * H4 * 4 +
                (with_backward ? L * 2 * (H * H4 * 2) + H * n->NHp * 2 : 0) + 8192;
  if (n->ops.need(need) || n->perms.need(2 * H4 * 4)) {
    delete n;
    return HSAD_ERR_NOMEM;
  }
  (void)hipMemset(n->ops.p, 0, need);
  char* p = n->ops.as<char>();
  auto take = [&](size_t bytes) {
    char* r = p;
    p += (bytes + 255) & ~(size_t)255;
    return r;
  };
  n->W1 = (bf16_t*)take(H * n->Fp * 2);
  if (n->nfc == 2) {
    n->W2 = (bf16_t*)take(H * H * 2);
    n->W2T = with_backward ? (bf16_t*)take(H * H * 2) : nullptr;
  }
  for (int l = 0; l < kMaxL; ++l) {
    n->Wih[l] = n->Whh[l] = n->Wcat16[l] = n->WihT[l] = n->WhhT[l] = nullptr;
    n->bg[l] = n->bias16[l] = nullptr;
  }
  for (int l = 0; l < n->L; ++l) {
    n->Wih[l] = (bf16_t*)take(H4 * H * 2);
    n->Whh[l] = (bf16_t*)take(H4 * H * 2);
    n->bg[l] = (float*)take(H4 * 4);
    n->Wcat16[l] = with_backward ? nullptr : (bf16_t*)take(H4 * 2 * H * 2);
    n->bias16[l] = with_backward ? nullptr : (float*)take(H4 * 4);
    n->WihT[l] = with_backward ? (bf16_t*)take(H * H4 * 2) : nullptr;
    n->WhhT[l] = with_backward ? (bf16_t*)take(H * H4 * 2) : nullptr;
  }
  n->Wheads = (bf16_t*)take((size_t)n->NH * H * 2);
  n->bheads = (float*)take(n->NHp * 4);
  n->WheadsT = with_backward ? (bf16_t*)take(H * n->NHp * 2) : nullptr;
  // row permutations of the LSTM weights: gate-blocked (32 units x [i f g o]) and gate16 (16 units x [i f g o])
  std::vector<int32_t> pm(2 * H4);
  for (int nb = 0; nb < (int)H / 32; ++nb)
    for (int g = 0; g < 4; ++g)
      for (int u = 0; u < 32; ++u) pm[nb * 128 + g * 32 + u] = g * (int)H + nb * 32 + u;
  for (int ub = 0; ub < (int)H / 16; ++ub)
    for (int g = 0; g < 4; ++g)
      for (int u = 0; u < 16; ++u) pm[H4 + ub * 64 + g * 16 + u] = g * (int)H + ub * 16 + u;
  n->perm32 = n->perms.as<int32_t>();
  n->perm16 = n->perm32 + H4;
  if (hipMemcpy(n->perm32, pm.data(), pm.size() * 4, hipMemcpyHostToDevice) != hipSuccess) {
    delete n;
    return afail(HSAD_ERR_HIP, "r2d2_net_create: permutation upload failed");
  }
  *out = n;
  return 0;
}

int hsad_r2d2_net_create(int in_dim, int hid_dim, int num_action, int hand_size, int with_backward, int device, hsad_r2d2_net** out) {
  return hsad_r2d2_net_create_ex(in_dim, hid_dim, num_action, hand_size, 1, 2, 0, with_backward, device, out);
}

void hsad_r2d2_net_destroy(hsad_r2d2_net* n) { delete n; }
int64_t hsad_r2d2_net_param_count(const hsad_r2d2_net* n) { return n ? (int64_t)n->n_param : 0; }
float* hsad_r2d2_net_params(hsad_r2d2_net* n) { return n ? n->flat : nullptr; }
int64_t hsad_r2d2_net_param_offset(const hsad_r2d2_net* n, int i) { return (n && i >= 0 && i <= n->np) ? (int64_t)n->off[i] : -1; }
int64_t hsad_r2d2_net_param_size(const hsad_r2d2_net* n, int i) { return (n && i >= 0 && i < n->np) ? (int64_t)net_tensor_elems(n, i) : -1; }
uint64_t hsad_r2d2_net_version(const hsad_r2d2_net* n) { return n ? n->version : 0; }
int hsad_r2d2_net_in_dim_padded(const hsad_r2d2_net* n) { return n ? n->Fp : 0; }

int hsad_r2d2_net_refresh(hsad_r2d2_net* n, void* stream) {
  if (!n) return afail(HSAD_ERR_INVALID, "null net");
  return net_refresh(n, (hipStream_t)stream);
}

// an acting step on checked arguments: hsad_r2d2_act, and with temp / row_key / sample_seed hsad_r2d2_act_soft (no target there)
static int act_step(hsad_r2d2_net* n, hsad_r2d2_net* target, int N, const float* priv_s, const void* priv_s_bf16, const float* legal_move,
                    const float* eps, const float* temp, const int64_t* row_key, uint64_t sample_seed, const float* h0, const float* c0,
                    const void* h0_bf16, uint64_t seed, uint64_t counter, int64_t* a, int64_t* greedy_a, float* h_out, float* c_out,
                    void* h_out_bf16, float* q_online_a, float* q_target_greedy, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  const int H = n->H, A = n->A, NH = n->NH;
  const bool hd_aligned = (size_t)N * NH * 4 % 16 == 0;
  PassWs w;
  CK(pass_ws(n, N, 2, 0, &w));
  CK(obs_bf16(n, N, priv_s, priv_s_bf16, &w, stream));
  StepOut so{}, st{};
  // (the bf16 copy of the new state goes straight into the caller's buffer, which must not alias h0_bf16: layer 1 still reads that)
  // both nets read the same observation: their input layers are ONE launch of two problems over a shared A operand
  const bool pair_in = q_target_greedy && target->F == n->F && target->H == H && target->A == A && n->nfc == 1 && target->nfc == 1;
  if (pair_in)
    CK(hsad_gemm_nt_bf16_pair(w.a16, w.a16, n->Fp, n->W1, target->W1, n->Fp, N, H, n->Fp, n->w(n->iB1), target->w(target->iB1), nullptr, nullptr, 0,
                              w.step[0], w.step[1], H, 1, stream));
  // ... so are the LSTM layers (one launch of two cell problems per layer) when both nets take the fused inference path ...
  const bool pair_trunk = pair_in && hd_aligned && N >= 1024 && n->Wcat16[0] && target->Wcat16[0] && !n->with_backward && !target->with_backward &&
                          n->L == target->L && !n->skip && !target->skip;
  if (pair_trunk || (pair_in && hd_aligned)) {
    if (pair_trunk) {
      CK(net_step_pair(n, target, N, h0, c0, (const bf16_t*)h0_bf16, h_out, c_out, w.step[0], w.step[1], &so, &st, s, (bf16_t*)h_out_bf16));
    } else {
      // ... and so are their head layers (N = A + 1 + 3 hand: one problem alone leaves half of the chip without a tile); the target's
      // trunk therefore runs before the online heads.  Same kernels on the same operands as the sequence below: identical bits.
      CK(net_step(n, N, w.a16, h0, c0, (const bf16_t*)h0_bf16, h_out, c_out, w.step[0], &so, s, (bf16_t*)h_out_bf16, true, true));
      const bf16_t* h16_shared = (const bf16_t*)h0_bf16;
      if (!h16_shared && so.h16_new) h16_shared = reinterpret_cast<const bf16_t*>(w.step[0] + (size_t)2 * N * H * 2);
      CK(net_step(target, N, w.a16, h0, c0, h16_shared, nullptr, nullptr, w.step[1], &st, s, nullptr, true));
    }
    CK(hsad_gemm_nt_bf16_pair(so.o16, st.o16, H, n->Wheads, target->Wheads, H, N, NH, H, n->bheads, target->bheads, w.hd[0], w.hd[1], NH, nullptr,
                              nullptr, 0, 0, stream));
    return hsad_act_select_q2(w.hd[0], w.hd[1], NH, legal_move, eps, N, A, seed, counter, a, greedy_a, q_online_a, q_target_greedy, w.scratch, stream);
  }
  CK(net_heads(n, N, nullptr, w.a16, h0, c0, (const bf16_t*)h0_bf16, h_out, c_out, &w, 0, &so, s, (bf16_t*)h_out_bf16, pair_in, true));
  // action, greedy action and Q_online(s, a) from one pass over the heads (same arithmetic as hsad_act_select + hsad_q_head); without a
  // temperature this is hsad_act_select_q
  CK(hsad_act_sample_q(w.hd[0], NH, legal_move, eps, temp, row_key, sample_seed, N, A, seed, counter, a, greedy_a, q_online_a, w.scratch, stream));
  if (q_target_greedy) {
    if (target->F != n->F || target->H != H || target->A != A) return afail(HSAD_ERR_INVALID, "r2d2_act: online / target shapes differ");
    // the target pass shares the bf16 casts of the observation and (fused path) of the hidden state
    const bf16_t* h16_shared = (const bf16_t*)h0_bf16;
    if (!h16_shared && so.h16_new) h16_shared = reinterpret_cast<const bf16_t*>(w.step[0] + (size_t)2 * N * H * 2);   // the cast net_step made
    CK(net_heads(target, N, nullptr, w.a16, h0, c0, h16_shared, nullptr, nullptr, &w, 1, &st, s, nullptr, pair_in));
    CK(hsad_q_at(w.hd[1], NH, legal_move, greedy_a, N, A, q_target_greedy, stream));
  }
  return 0;
}

// R2D2Agent.act (pyhanabi/r2d2.py:247-303) for N rows (one row per (game, player)): eps-greedy action, greedy action, new
// hidden state.  q_online_a / q_target_greedy (both or neither; `target` required with them): Q_online(s, a) of the pass just
// run and Q_target(s, greedy_a) from one target-net pass -- what compute_priority needs from this time step.
int hsad_r2d2_act(hsad_r2d2_net* online, hsad_r2d2_net* target, int N, const float* priv_s, const void* priv_s_bf16,
                  const float* legal_move, const float* eps, const float* h0, const float* c0, const void* h0_bf16, uint64_t seed, uint64_t counter,
                  int64_t* a, int64_t* greedy_a, float* h_out, float* c_out, void* h_out_bf16, float* q_online_a,
                  float* q_target_greedy, void* stream) {
  if (online) CK(net_wait(online, (hipStream_t)stream));
  if (target) CK(net_wait(target, (hipStream_t)stream));
  if (!online || (!priv_s && !priv_s_bf16) || !legal_move || !h0 || !c0 || !a || !greedy_a || !h_out || !c_out || N < 1)
    return afail(HSAD_ERR_INVALID, "r2d2_act: null argument");
  if (q_target_greedy && (!q_online_a || !target))
    return afail(HSAD_ERR_INVALID, "r2d2_act: q_target_greedy needs q_online_a and the target net");
  if (q_online_a && online->skip)
    return afail(HSAD_ERR_INVALID, "r2d2_act: cached Q-values are undefined for a skip_connect net -- R2D2Net.act adds the skip connection, "
                 "R2D2Net.forward (what compute_priority evaluates) ignores it (pyhanabi/r2d2.py:74-75 vs 99-105); use hsad_r2d2_compute_priority");
  if (target && (target->L != online->L || target->H != online->H)) return afail(HSAD_ERR_INVALID, "r2d2_act: online / target shapes differ");
  if (h_out_bf16 && h_out_bf16 == h0_bf16) return afail(HSAD_ERR_INVALID, "r2d2_act: h_out_bf16 must not alias h0_bf16");
  return act_step(online, target, N, priv_s, priv_s_bf16, legal_move, eps, nullptr, nullptr, 0, h0, c0, h0_bf16, seed, counter, a, greedy_a, h_out,
                  c_out, h_out_bf16, q_online_a, q_target_greedy, stream);
}

// hsad_r2d2_act(online = net, target = NULL) with the sampling tail (hsad_act_sample_q): the same step, so the new state and -- with
// temp == NULL -- every output are that call's bits
int hsad_r2d2_act_soft(hsad_r2d2_net* net, int N, const float* priv_s, const void* priv_s_bf16, const float* legal_move, const float* eps,
                       const float* temp, const int64_t* row_key, uint64_t sample_seed, const float* h0, const float* c0,
                       const void* h0_bf16, uint64_t seed, uint64_t counter, int64_t* a, int64_t* greedy_a, float* h_out, float* c_out,
                       void* h_out_bf16, float* q_online_a, void* stream) {
  if (net) CK(net_wait(net, (hipStream_t)stream));
  if (!net || (!priv_s && !priv_s_bf16) || !legal_move || !h0 || !c0 || !a || !greedy_a || !h_out || !c_out || N < 1)
    return afail(HSAD_ERR_INVALID, "r2d2_act_soft: null argument");
  if (q_online_a && net->skip)
    return afail(HSAD_ERR_INVALID, "r2d2_act_soft: cached Q-values are undefined for a skip_connect net (see hsad_r2d2_act)");
  if (h_out_bf16 && h_out_bf16 == h0_bf16) return afail(HSAD_ERR_INVALID, "r2d2_act_soft: h_out_bf16 must not alias h0_bf16");
  return act_step(net, nullptr, N, priv_s, priv_s_bf16, legal_move, eps, temp, row_key, sample_seed, h0, c0, h0_bf16, seed, counter, a, greedy_a,
                  h_out, c_out, h_out_bf16, q_online_a, nullptr, stream);
}

// Q_target(s, greedy_a) alone: the target-net half of an acting step as its own call, so that a caller can issue the env step
// (which only needs the online half's actions) before it and run the two side by side (actor.DeviceActor does)
int hsad_r2d2_target_q(hsad_r2d2_net* target, int N, const float* priv_s, const void* priv_s_bf16, const float* legal_move,
                       const float* h0, const float* c0, const void* h0_bf16, const int64_t* greedy_a, float* q_target_greedy, void* stream) {
  if (target) CK(net_wait(target, (hipStream_t)stream));
  if (!target || (!priv_s && !priv_s_bf16) || !legal_move || !h0 || !c0 || !greedy_a || !q_target_greedy || N < 1)
    return afail(HSAD_ERR_INVALID, "r2d2_target_q: null argument");
  PassWs w;
  CK(pass_ws(target, N, 1, 0, &w));
  StepOut st{};
  CK(net_heads(target, N, priv_s, priv_s_bf16, h0, c0, (const bf16_t*)h0_bf16, nullptr, nullptr, &w, 0, &st, (hipStream_t)stream));
  return hsad_q_at(w.hd[0], target->NH, legal_move, greedy_a, N, target->A, q_target_greedy, stream);
}

// Q_net(s, action) [N] for one step from the carried hidden state
static int net_q_of(hsad_r2d2_net* n, int N, const float* priv_s, const float* legal, const int64_t* action, const float* h0,
                    const float* c0, float* qa, int64_t* greedy_out, hipStream_t s) {
  void* stream = (void*)s;
  const size_t q_b = ((size_t)N * n->A * 4 + 15) & ~(size_t)15;
  PassWs w;
  CK(pass_ws(n, N, 2, q_b + (size_t)N * 8, &w));
  float* q = (float*)w.extra;
  int64_t* junk = (int64_t*)(w.extra + q_b);
  StepOut so{};
  // the greedy action of compute_priority comes from R2D2Agent.greedy_act = R2D2Net.act (skip connection applies), Q(s, a) from
  // R2D2Net.forward (it does not): pyhanabi/r2d2.py:234-244, 340-345
  CK(net_heads(n, N, priv_s, nullptr, h0, c0, nullptr, nullptr, nullptr, &w, 0, &so, s, nullptr, false, greedy_out != nullptr));
  if (greedy_out) CK(hsad_act_select(w.hd[0], n->NH, legal, nullptr, N, n->A, 0, 0, junk, greedy_out, w.scratch, stream));
  if (qa) CK(hsad_q_head(w.hd[0], n->NH, legal, action, N, n->A, q, qa, nullptr, w.scratch, stream));
  return 0;
}

// Q_net(s, action) [N] for one step from the carried hidden state (one network pass; the pieces compute_priority is made of)
int hsad_r2d2_q_of(hsad_r2d2_net* net, int N, const float* priv_s, const float* legal_move, const int64_t* action, const float* h0,
                   const float* c0, float* qa, void* stream) {
  if (net) CK(net_wait(net, (hipStream_t)stream));
  if (!net || !priv_s || !legal_move || !action || !h0 || !c0 || !qa || N < 1) return afail(HSAD_ERR_INVALID, "r2d2_q_of: null argument");
  return net_q_of(net, N, priv_s, legal_move, action, h0, c0, qa, nullptr, (hipStream_t)stream);
}

// R2D2Agent.compute_priority (pyhanabi/r2d2.py:305-361): |r + bootstrap * gamma^n * Q_target(s', argmax_a' adv_online(s')) - Q_online(s, a)|
// rows are (game, player) pairs; num_player > 1 = VDN: Q summed over the players of a game, reward / bootstrap / priority per game.
// next_greedy_a (may be NULL): argmax_a' adv_online(s') when the caller already has it (the act() of the same iteration).
int hsad_r2d2_compute_priority(hsad_r2d2_net* online, hsad_r2d2_net* target, int N, int num_player, const float* priv_s,
                               const float* legal_move, const int64_t* a, const float* next_priv_s, const float* next_legal_move,
                               const float* h0, const float* c0, const float* next_h0, const float* next_c0, const float* reward,
                               const float* bootstrap, int multi_step, double gamma, const int64_t* next_greedy_a, float* priority,
                               void* stream) {
  if (online) CK(net_wait(online, (hipStream_t)stream));
  if (target) CK(net_wait(target, (hipStream_t)stream));
  if (!online || !target || !priv_s || !legal_move || !a || !next_priv_s || !next_legal_move || !h0 || !c0 || !next_h0 || !next_c0 ||
      !reward || !bootstrap || !priority || N < 1 || num_player < 1 || N % num_player)
    return afail(HSAD_ERR_INVALID, "r2d2_compute_priority: bad arguments");
  hipStream_t s = (hipStream_t)stream;
  const int n_game = N / num_player;
  CK(online->scratch.need((size_t)N * (4 + 4 + 8) + (size_t)n_game * 8 + 64));
  float* qa = online->scratch.as<float>();
  float* tqa = qa + N;
  int64_t* na = reinterpret_cast<int64_t*>(tqa + N);
  float* sq = reinterpret_cast<float*>(na + N);
  CK(net_q_of(online, N, priv_s, legal_move, a, h0, c0, qa, nullptr, s));
  if (!next_greedy_a) {
    CK(net_q_of(online, N, next_priv_s, next_legal_move, nullptr, next_h0, next_c0, nullptr, na, s));
    next_greedy_a = na;
  }
  CK(net_q_of(target, N, next_priv_s, next_legal_move, next_greedy_a, next_h0, next_c0, tqa, nullptr, s));
  int n_out = N;
  if (num_player > 1) {
    n_out = n_game;
    hipLaunchKernelGGL(sum_players_kernel, dim3((n_out + 255) / 256), dim3(256), 0, s, qa, n_out, num_player, sq);
    hipLaunchKernelGGL(sum_players_kernel, dim3((n_out + 255) / 256), dim3(256), 0, s, tqa, n_out, num_player, sq + n_out);
    qa = sq;
    tqa = sq + n_out;
  }
  return hsad_nstep_priority(qa, tqa, reward, bootstrap, multi_step, gamma, n_out, priority, stream);
}

}  // extern "C"
