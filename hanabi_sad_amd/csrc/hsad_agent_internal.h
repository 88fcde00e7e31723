// hsad_agent_internal.h — what the composite entry points of hsad_agent.hip (nets, act, q_of, compute_priority) and hsad_learner.hip (the
// learner) share: error plumbing, the grow-only device buffer, the net and its operand refresh.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <string>

#include "hsad.h"

extern "C" int hsad_internal_set_error(int code, const char* msg);

namespace {

int afail(int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  return hsad_internal_set_error(code, buf);
}
#define HIP_TRY(expr)                                                                          \
  do {                                                                                         \
    hipError_t e_ = (expr);                                                                    \
    if (e_ != hipSuccess) return afail(HSAD_ERR_HIP, "%s failed: %s", #expr, hipGetErrorString(e_)); \
  } while (0)
#define CK(expr)            \
  do {                      \
    const int rc_ = (expr); \
    if (rc_) return rc_;    \
  } while (0)

typedef unsigned short bf16_t;
inline int pad64(int k) { return (k + 63) / 64 * 64; }

constexpr int kMaxL = 3;     // nn.LSTM(num_layers): the reference's --num_lstm_layer (pyhanabi/selfplay.py:50), 1..3 here
constexpr int kMaxP = 4 + 4 * kMaxL + 6;

// grow-only device buffer
struct Buf {
  void* p = nullptr;
  size_t cap = 0;
  int need(size_t bytes) {
    if (bytes <= cap) return 0;
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
    if (hipMalloc(&p, bytes) != hipSuccess) return afail(HSAD_ERR_NOMEM, "hipMalloc of %zu bytes failed", bytes);
    cap = bytes;
    return 0;
  }
  template <typename T>
  T* as() const {
    return reinterpret_cast<T*>(p);
  }
  ~Buf() {
    if (p) (void)hipFree(p);
  }
};

// VDN: Q summed over the players of a game (compute_priority and the learner's loss)
__global__ void sum_players_kernel(const float* __restrict__ x, int n_out, int P, float* __restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_out) return;
  float s = 0.f;
  for (int p = 0; p < P; ++p) s += x[(size_t)i * P + p];
  out[i] = s;
}

inline int transpose16(const bf16_t* src, int R, int C, int lds, bf16_t* dst, int ldd, float* csum, float* csum2, const int32_t* cmap, void* st) {
  if (csum) return hsad_transpose_bf16_colsum(src, R, C, lds, dst, ldd, csum, csum2, cmap, st);
  return hsad_transpose_bf16(src, R, C, lds, dst, ldd, st);
}

}  // namespace

// R2D2Net(in_dim, hid_dim, out_dim, num_lstm_layer, hand_size, num_fc_layer, skip_connect) (pyhanabi/r2d2.py:22-57).  Parameter
// tensors in state_dict order of the module tree: net.0.*, [net.2.*], lstm.{weight_ih,weight_hh,bias_ih,bias_hh}_l{k}, then the heads
// as [fc_a | fc_v | pred] weights and [fc_a | fc_v | pred] biases (contiguous [NH, H] / [NH] blocks).
struct hsad_r2d2_net {
  int F, Fp, H, A, NP, NH, NHp, device;
  int nfc = 1, L = 2;
  bool skip = false;
  bool with_backward;
  size_t n_param;
  int np = 0;                          // parameter tensors
  size_t off[kMaxP + 1];
  std::string names[kMaxP];
  int iW1, iB1, iW2 = -1, iB2 = -1, iWih[kMaxL], iWhh[kMaxL], iBih[kMaxL], iBhh[kMaxL], iWA, iWV, iWP, iBA, iBV, iBP;
  float* flat = nullptr;     // fp32 masters, all tensors back to back
  bool owns_flat = true;
  Buf flat_buf, ops, perms, scratch;
  bf16_t *W1, *W2 = nullptr, *W2T = nullptr, *Wih[kMaxL], *Whh[kMaxL], *Wheads, *Wcat16[kMaxL], *WihT[kMaxL], *WhhT[kMaxL], *WheadsT;
  float *bg[kMaxL], *bheads, *bias16[kMaxL];
  int32_t *perm32, *perm16;
  uint64_t version = 0;
  // split refresh (net_refresh_split): the LSTM operands are re-derived on a side stream; whoever reads them next waits for this
  hipEvent_t ev_refresh = nullptr;
  bool split_pending = false;
  // acting workspace (grows with the row count)
  Buf ws;
  float* w(int i) const { return flat + off[i]; }
  ~hsad_r2d2_net() {
    if (ev_refresh) (void)hipEventDestroy(ev_refresh);
  }
};

// (hsad_agent.hip)
int net_wait(hsad_r2d2_net* n, hipStream_t s);
int net_refresh(hsad_r2d2_net* n, hipStream_t s);
int net_refresh_split(hsad_r2d2_net* n, hipStream_t s, hipStream_t side, hipEvent_t ev_tmp);
