// csrc/r2d2/act_sample.inc -- included by csrc/hsad_r2d2.hip inside its anonymous namespace, after act.inc.
// the acting tail of a network seat that plays its softmax policy: act_select_q_kernel's row, and on the rows with a temperature > 0
// an action sampled from the softmax over the legal advantages (the distribution clone_tail_kernel fits) instead of their argmax.
// The draws and Pick are hsad_act_sample.h's, which the CPU suite compiles alone.
// ---------------------------------------------------------------------------------------------------
// Same shape as act_select_q_kernel: after adv_min_kernel, a block stages its R rows of heads / legal through LDS and reduces the
// per-block minima itself; one row per lane.  greedy_out is act_select_q_kernel's expression (global minimum shift, lowest-index ties);
// a row with temp <= 0 (or temp == NULL) is that kernel's row, bit for bit.  On a row with temp > 0 the exploration draw comes first and
// takes the uniform legal action it takes there; otherwise a = Pick(advantages, legal, temp, u).  The walk over the A columns runs on
// the lane's own LDS rows and registers: lanes of a wave leave it at different columns, nothing is shared, no atomics.
__global__ __launch_bounds__(256) void act_sample_q_kernel(const float* __restrict__ heads, int ldh, const float* __restrict__ legal,
                                                           const float* __restrict__ eps, const float* __restrict__ temp,
                                                           const int64_t* __restrict__ row_key, unsigned long long sample_seed,
                                                           const float* __restrict__ block_min, int nb, int N, int A,
                                                           unsigned long long seed, unsigned long long counter,
                                                           int64_t* __restrict__ a_out, int64_t* __restrict__ greedy_out,
                                                           float* __restrict__ qa_out, int R) {
  extern __shared__ float s_act[];
  float* s_h = s_act;                    // [R][ldh]
  float* s_l = s_act + R * ldh;          // [R][A]
  __shared__ float s_red[256];
  const int tid = threadIdx.x, m0 = blockIdx.x * R, rows = min(R, N - m0);
  for (int i = tid; i < rows * ldh; i += 256) s_h[i] = heads[(size_t)m0 * ldh + i];
  for (int i = tid; i < rows * A; i += 256) s_l[i] = legal[(size_t)m0 * A + i];
  float mn = 3.4e38f;
  for (int i = tid; i < nb; i += 256) mn = fminf(mn, block_min[i]);
  s_red[tid] = mn;
  __syncthreads();
  for (int k = 128; k > 0; k >>= 1) {
    if (tid < k) s_red[tid] = fminf(s_red[tid], s_red[tid + k]);
    __syncthreads();
  }
  mn = s_red[0];
  if (tid >= rows) return;
  const int m = m0 + tid;
  const float* h = s_h + tid * ldh;
  const float* lg = s_l + tid * A;
  float best = -3.4e38f, mean = 0.f;
  int bi = 0, nlegal = 0;
  for (int j = 0; j < A; ++j) {
    const float l = lg[j];
    const float sc = (1.f + h[j] - mn) * l;
    if (sc > best) {
      best = sc;
      bi = j;
    }
    nlegal += l != 0.f;
    mean += h[j] * l;
  }
  greedy_out[m] = bi;
  int act = bi;
  const float e = eps ? eps[m] : 0.f;
  const float tau = temp ? temp[m] : 0.f;
  if ((e > 0.f || tau > 0.f) && nlegal > 0) {
    const unsigned long long hh = as_eps_hash(seed, (unsigned long long)m, counter);
    bool explore = false;
    if (e > 0.f && as_uniform(hh) < e) {
      explore = true;
      int k = as_eps_index(hh, nlegal);
      for (int j = 0; j < A; ++j)
        if (lg[j] != 0.f && k-- == 0) {
          act = j;
          break;
        }
    }
    if (!explore && tau > 0.f) {
      const unsigned long long hs = row_key ? as_sample_hash_keyed(sample_seed, row_key[m]) : as_sample_hash(hh);
      act = as_pick(h, lg, A, tau, as_uniform(hs));
    }
  }
  a_out[m] = act;
  if (qa_out) {
    mean /= (float)A;
    qa_out[m] = h[A] + h[act] * lg[act] - mean;     // act_select_q_kernel's (= q_at_kernel's) expression at the chosen action
  }
}
