// clone_value.inc — behaviour cloning with a value term: clone_loss.inc's cross-entropy of the recorded action PLUS the Huber regression of
// Q(o_t, a_t) on the return-to-go of the recorded game (a Monte-Carlo sample of the teacher's Q, the quantity the TD loss bootstraps towards).
// A net fitted with both plays the teacher's greedy move and carries Q-values on the scale of the returns: the supervised half of learning
// from demonstrations.  clone_tail_kernel is untouched; with value_weight == 0 and policy_weight == 1 this kernel writes its bits.

// ---------------------------------------------------------------------------------------------------
// The shape of clone_tail_kernel: one block per sequence b, the threads stride over the steps t (any T), row m = t B + b; z, l, act, valid, bad,
// xent, p_j, hits, decisions exactly as there (the single-legal special case included).  For every valid row that is not bad, additionally
//   al_j = z_j l_j, v = heads[m ldh + A], q = v + al_act - (sum_j al_j) / A       (q_head_kernel's arithmetic: the dueling head at the action)
//   e = ret[m] - q, hub = |e| < 1 ? e e / 2 : |e| - 1/2, g = -clamp(e, -1, 1)     (td_loss_kernel's Huber and its derivative)
// With s = weight[b] / B:
//   dheads[m ldo + j] = bf16(s (policy_weight (p_j - delta_{j, act}) [>= 2 legal] + value_weight g l_j (delta_{j, act} - 1/A)))   for j < A
//   dheads[m ldo + A] = bf16(s value_weight g);  columns A + 1 .. ldo - 1 are 0
// (the two terms are summed in fp32 and rounded once; an illegal column is +0).  A single-legal row carries the value term alone: the off-turn
// no-op has a Q too.  Invalid and bad rows are all-zero bits and read neither ret nor the logits nor (past seq_len) a legal mask.
// loss[b] = sum_t xent and vloss[b] = sum_t hub, each in ascending t by one thread; steps[b] = valid rows that are not bad; the counters are
// integer sums (wave shuffles, then one LDS word per wave and counter): the same bits run to run, no float atomics.
// value_weight == 0 is a uniform branch that reads no ret and no value column and writes no vloss.
// ---------------------------------------------------------------------------------------------------
struct CloneValueArgs {
  const float *heads, *legal, *ret, *seq_len, *weight;
  const int64_t* action;
  int ldh, T, B, A;
  float policy_weight, value_weight;
  float *loss, *vloss;
  int32_t *hits, *decisions, *bad, *steps;
  bf16_t* dheads;      // NULL = no gradient
  int ldo;
};
constexpr int kCloneValueThreads = 128;
constexpr int kCloneValueWaves = kCloneValueThreads / 64;
__global__ __launch_bounds__(kCloneValueThreads) void clone_value_tail_kernel(CloneValueArgs p) {
  extern __shared__ __attribute__((aligned(16))) float s_cv[];
  float* s_x = s_cv;                                             // [T] cross-entropy of step t
  float* s_h = s_cv + p.T;                                       // [T] Huber term of step t
  int* s_cnt = reinterpret_cast<int*>(s_cv + 2 * p.T);           // [4][waves] hits | decisions | bad | steps
  const int b = blockIdx.x, tid = threadIdx.x, nt = blockDim.x, T = p.T, B = p.B, A = p.A;
  const bool with_value = p.value_weight != 0.f;                 // (uniform)
  const float len = p.seq_len[b];
  const float scale = p.dheads ? p.weight[b] / (float)B : 0.f;
  const float sp = scale * p.policy_weight, sv = scale * p.value_weight;
  const float invA = 1.f / (float)A;
  int n_hit = 0, n_dec = 0, n_bad = 0, n_step = 0;
  for (int t = tid; t < T; t += nt) {
    const size_t m = (size_t)t * B + b;
    const float* z = p.heads + m * p.ldh;
    const float* lg = p.legal + m * A;
    bf16_t* o = p.dheads ? p.dheads + m * p.ldo : nullptr;
    const bool valid = (float)t < len;
    const int64_t act64 = p.action[m];
    const int act = (act64 >= 0 && act64 < A) ? (int)act64 : -1;
    float xent = 0.f, hub = 0.f;
    bool grad_row = false;
    if (valid) {
      if (act < 0 || lg[act] == 0.f) {
        ++n_bad;
      } else {
        ++n_step;
        float mx = -3.4e38f;
        int bi = 0, nlegal = 0;
        for (int j = 0; j < A; ++j)
          if (lg[j] != 0.f) {
            ++nlegal;
            if (z[j] > mx) mx = z[j], bi = j;      // (strict: a tie keeps the lowest index)
          }
        float s = 1.f;
        if (nlegal >= 2) {
          s = 0.f;
          for (int j = 0; j < A; ++j)
            if (lg[j] != 0.f) s += __expf(z[j] - mx);
          xent = __logf(s) - (z[act] - mx);
          ++n_dec;
          n_hit += bi == act;
        }
        if (!with_value) {
          if (o && nlegal >= 2) {      // clone_tail_kernel's row, its expression: the same bits at policy_weight 1
            const float inv = 1.f / s;
            for (int j = 0; j < A; ++j) o[j] = lg[j] != 0.f ? f2bf(sp * (__expf(z[j] - mx) * inv - (j == act ? 1.f : 0.f))) : (bf16_t)0;
            for (int j = A; j < p.ldo; ++j) o[j] = 0;
            grad_row = true;
          }
        } else {
          float mean = 0.f;
          for (int j = 0; j < A; ++j) mean += z[j] * lg[j];
          mean /= (float)A;
          const float q = z[A] + z[act] * lg[act] - mean;
          const float e = p.ret[m] - q;
          const float ae = fabsf(e);
          hub = ae < 1.f ? 0.5f * e * e : ae - 0.5f;
          if (o) {
            const float g = -fminf(fmaxf(e, -1.f), 1.f);
            const float inv = 1.f / s;
            const bool multi = nlegal >= 2;
            for (int j = 0; j < A; ++j) {
              const float d = j == act ? 1.f : 0.f;
              const float pol = multi ? p.policy_weight * (__expf(z[j] - mx) * inv - d) : 0.f;
              o[j] = lg[j] != 0.f ? f2bf(scale * (pol + p.value_weight * g * lg[j] * (d - invA))) : (bf16_t)0;
            }
            o[A] = f2bf(sv * g);
            for (int j = A + 1; j < p.ldo; ++j) o[j] = 0;
            grad_row = true;
          }
        }
      }
    }
    if (o && !grad_row)
      for (int j = 0; j < p.ldo; ++j) o[j] = 0;
    s_x[t] = xent;
    if (with_value) s_h[t] = hub;
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
