// clone_loss.inc — behaviour cloning on the head outputs: cross-entropy of the recorded action under softmax over the LEGAL advantage
// columns, its gradient, and the agreement counters.  Under the dueling head softmax over legal advantages is softmax over legal Q (the value
// and the mean cancel), and its argmax is what hsad_r2d2_act plays greedily, so a net fitted with this loss is an R2D2 agent as it stands.
// The value column gets no gradient from cloning.

// ---------------------------------------------------------------------------------------------------
// The shape of loss_tail_kernel: one block per sequence b, the threads stride over the steps t (any T).  Row m = t B + b:
//   z_j = heads[m ldh + j] (j < A), l_j = legal[m A + j] (0 / 1), act = action[m], valid = t < seq_len[b] (td_loss_kernel's mask)
//   bad    = valid and (act outside [0, A) or l_act == 0): contributes nothing, counted in bad[b]
//   xent   = log sum_legal exp(z_j - mx) - (z_act - mx), mx = max_legal z_j;  p_j = l_j exp(z_j - mx) / sum
//   dheads[m ldo + j] = bf16(weight[b] / B (p_j - delta_{j, act})) for j < A; the value column A and every column up to ldo are 0
// A step with ONE legal action (every off-turn step: the no-op) is exactly xent = 0 and an all-zero row -- special-cased, the fast exp / log
// are not asked to give 1 and 0.  Invalid and bad rows are all zeros and read neither their logits nor (past seq_len) a legal mask that may
// be all zero: no NaN.  loss[b] = sum_t xent in ascending t by one thread; the counters are integer sums: the same bits run to run.
// decisions[b] = valid, not bad steps with >= 2 legal actions; hits[b] = those whose argmax_legal z_j (ties: lowest index) is act.
// ---------------------------------------------------------------------------------------------------
struct CloneTailArgs {
  const float *heads, *legal, *seq_len, *weight;
  const int64_t* action;
  int ldh, T, B, A;
  float* loss;
  int32_t *hits, *decisions, *bad;
  bf16_t* dheads;      // NULL = no gradient
  int ldo;
};
__global__ __launch_bounds__(128) void clone_tail_kernel(CloneTailArgs p) {
  extern __shared__ __attribute__((aligned(16))) float s_ct[];
  float* s_x = s_ct;                                             // [T] cross-entropy of step t
  int* s_cnt = reinterpret_cast<int*>(s_ct + p.T);               // [3][blockDim] hits | decisions | bad
  const int b = blockIdx.x, tid = threadIdx.x, nt = blockDim.x, T = p.T, B = p.B, A = p.A;
  const float len = p.seq_len[b];
  const float scale = p.dheads ? p.weight[b] / (float)B : 0.f;
  int n_hit = 0, n_dec = 0, n_bad = 0;
  for (int t = tid; t < T; t += nt) {
    const size_t m = (size_t)t * B + b;
    const float* z = p.heads + m * p.ldh;
    const float* lg = p.legal + m * A;
    bf16_t* o = p.dheads ? p.dheads + m * p.ldo : nullptr;
    const bool valid = (float)t < len;
    const int64_t act64 = p.action[m];
    const int act = (act64 >= 0 && act64 < A) ? (int)act64 : -1;
    float xent = 0.f;
    bool grad_row = false;
    if (valid) {
      if (act < 0 || lg[act] == 0.f) {
        ++n_bad;
      } else {
        float mx = -3.4e38f;
        int bi = 0, nlegal = 0;
        for (int j = 0; j < A; ++j)
          if (lg[j] != 0.f) {
            ++nlegal;
            if (z[j] > mx) mx = z[j], bi = j;      // (strict: a tie keeps the lowest index)
          }
        if (nlegal >= 2) {
          float s = 0.f;
          for (int j = 0; j < A; ++j)
            if (lg[j] != 0.f) s += __expf(z[j] - mx);
          xent = __logf(s) - (z[act] - mx);
          ++n_dec;
          n_hit += bi == act;
          if (o) {
            const float inv = 1.f / s;
            for (int j = 0; j < A; ++j) o[j] = lg[j] != 0.f ? f2bf(scale * (__expf(z[j] - mx) * inv - (j == act ? 1.f : 0.f))) : (bf16_t)0;
            for (int j = A; j < p.ldo; ++j) o[j] = 0;
            grad_row = true;
          }
        }
      }
    }
    if (o && !grad_row)
      for (int j = 0; j < p.ldo; ++j) o[j] = 0;
    s_x[t] = xent;
  }
  s_cnt[tid] = n_hit;
  s_cnt[nt + tid] = n_dec;
  s_cnt[2 * nt + tid] = n_bad;
  __syncthreads();
  for (int k = nt / 2; k > 0; k >>= 1) {
    if (tid < k) {
      s_cnt[tid] += s_cnt[tid + k];
      s_cnt[nt + tid] += s_cnt[nt + tid + k];
      s_cnt[2 * nt + tid] += s_cnt[2 * nt + tid + k];
    }
    __syncthreads();
  }
  if (tid == 0) {
    float total = 0.f;
    for (int t = 0; t < T; ++t) total += s_x[t];      // ascending t (aux_xent_kernel's order)
    p.loss[b] = total;
    p.hits[b] = s_cnt[0];
    p.decisions[b] = s_cnt[nt];
    p.bad[b] = s_cnt[2 * nt];
  }
}
