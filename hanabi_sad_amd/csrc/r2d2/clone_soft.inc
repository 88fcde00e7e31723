// clone_soft.inc — behaviour cloning against a TARGET DISTRIBUTION per row instead of the one recorded move: clone_value.inc's row with one more
// input, target float32 [M, A], a probability row pi for every row m = t B + b.  What a search knows about a position -- a mean playout score
// for every legal action -- or a teacher's softmax policy reaches the net as cross-entropy against that row (clone.soft_targets makes it).
// clone_tail_kernel and clone_value_tail_kernel are untouched; where a target row is the one-hot of action[m] this kernel writes the bits of
// clone_value_tail_kernel.

// ---------------------------------------------------------------------------------------------------
// The shape of clone_value_tail_kernel: one block per sequence b, the threads stride over the steps t (any T), row m = t B + b, the row itself
// is cs_row of csrc/hsad_clone_soft.h (which the CPU suite compiles on its own):
//   sigma = sum_{legal j} pi_j,  xent = sigma log S - sum_{legal j} pi_j (z_j - mx),  policy gradient policy_weight (sigma p_j - pi_j)
// summed in fp32 with the unchanged value term (it still reads action[m] and ret[m]) and rounded to bf16 once.  hits and decisions are still
// defined against action[m].  A valid row is bad -- counted, all-zero gradient bits, nothing else -- when action[m] is bad by the siblings'
// rule, a pi_j is negative or NaN, an illegal column carries mass, or |sigma - 1| > 1e-3.  Rows past seq_len read no target.
// loss[b] and vloss[b] are sums in ascending t by one thread over per-step terms in LDS, the counters integer sums by wave shuffles: the same
// bits run to run, no float atomics.
// ---------------------------------------------------------------------------------------------------
struct CloneSoftArgs {
  const float *heads, *legal, *target, *ret, *seq_len, *weight;
  const int64_t* action;
  int ldh, T, B, A;
  float policy_weight, value_weight;
  float *loss, *vloss;
  int32_t *hits, *decisions, *bad, *steps;
  bf16_t* dheads;      // NULL = no gradient
  int ldo;
};
constexpr int kCloneSoftThreads = 128;
constexpr int kCloneSoftWaves = kCloneSoftThreads / 64;
__global__ __launch_bounds__(kCloneSoftThreads) void clone_soft_tail_kernel(CloneSoftArgs p) {
  extern __shared__ __attribute__((aligned(16))) float s_cs[];
  float* s_x = s_cs;                                             // [T] cross-entropy of step t
  float* s_h = s_cs + p.T;                                       // [T] Huber term of step t
  int* s_cnt = reinterpret_cast<int*>(s_cs + 2 * p.T);           // [4][waves] hits | decisions | bad | steps
  const int b = blockIdx.x, tid = threadIdx.x, nt = blockDim.x, T = p.T, B = p.B, A = p.A;
  const bool with_value = p.value_weight != 0.f;                 // (uniform)
  const float len = p.seq_len[b];
  const float scale = p.dheads ? p.weight[b] / (float)B : 0.f;
  int n_hit = 0, n_dec = 0, n_bad = 0, n_step = 0;
  for (int t = tid; t < T; t += nt) {
    const size_t m = (size_t)t * B + b;
    bf16_t* o = p.dheads ? p.dheads + m * p.ldo : nullptr;
    cs_row_out r{0.f, 0.f, 0, 0, 0, 0, false};
    if ((float)t < len)
      r = cs_row(p.heads + m * p.ldh, p.legal + m * A, p.target + m * A, A, p.action[m], with_value ? p.ret[m] : 0.f, p.policy_weight,
                 p.value_weight, scale, o != nullptr, p.ldo, [o](int j, float v) { o[j] = f2bf(v); });
    n_hit += r.hit, n_dec += r.dec, n_bad += r.bad, n_step += r.step;
    if (o && !r.grad_row)
      for (int j = 0; j < p.ldo; ++j) o[j] = 0;
    s_x[t] = r.xent;
    if (with_value) s_h[t] = r.hub;
  }
  // integer sums: inside a wave by shuffles (no LDS, no barrier), then one word per wave and counter
  for (int k = 32; k > 0; k >>= 1) {
    n_hit += __shfl_down(n_hit, k, 64);
    n_dec += __shfl_down(n_dec, k, 64);
    n_bad += __shfl_down(n_bad, k, 64);
    n_step += __shfl_down(n_step, k, 64);
  }
  const int wave = tid >> 6, nw = (nt + 63) >> 6;
  if ((tid & 63) == 0) {
    s_cnt[wave] = n_hit;
    s_cnt[nw + wave] = n_dec;
    s_cnt[2 * nw + wave] = n_bad;
    s_cnt[3 * nw + wave] = n_step;
  }
  __syncthreads();
  if (tid == 0) {
    float total = 0.f;
    for (int t = 0; t < T; ++t) total += s_x[t];      // ascending t (clone_tail_kernel's order)
    p.loss[b] = total;
    if (with_value) {
      float vtotal = 0.f;
      for (int t = 0; t < T; ++t) vtotal += s_h[t];
      p.vloss[b] = vtotal;
    }
    int c[4] = {0, 0, 0, 0};
    for (int w = 0; w < nw; ++w)
      for (int k = 0; k < 4; ++k) c[k] += s_cnt[k * nw + w];
    p.hits[b] = c[0];
    p.decisions[b] = c[1];
    p.bad[b] = c[2];
    p.steps[b] = c[3];
  }
}
