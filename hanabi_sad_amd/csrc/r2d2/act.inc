// csrc/r2d2/act.inc -- included by csrc/hsad_r2d2.hip inside its anonymous namespace (ONE translation unit: the kernels share the
// file-local helpers of common.inc and the host launchers in hsad_r2d2.hip).
// the acting tail: epsilon-greedy action selection with cached Q-values, per-row Q lookups, state zeroing of ended games, n-step priority
// ---------------------------------------------------------------------------------------------------
// R2D2Agent.act tail (r2d2.py:235-277): greedy by ADVANTAGE only, legal_adv = (1 + adv - min(adv)) * legal with the
// global min, uniform-random legal action, eps-greedy mix; on rows with a temperature, an action sampled from the softmax over the legal
// advantages.  The row itself -- argmax, draws, Q(s, a) -- is as_tail_row / as_q_at of csrc/hsad_act_sample.h, which the CPU suite
// compiles alone; the kernels here bring a row and the global minimum to it and store what it returns.
// ---------------------------------------------------------------------------------------------------
__global__ void adv_min_kernel(const float* __restrict__ heads, int ldh, int N, int A, float* __restrict__ block_min) {
  __shared__ float smin[256];
  const int m = blockIdx.x * blockDim.x + threadIdx.x;
  float mn = 3.4e38f;
  if (m < N)
    for (int j = 0; j < A; ++j) mn = fminf(mn, heads[(size_t)m * ldh + j]);
  smin[threadIdx.x] = mn;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (threadIdx.x < s) smin[threadIdx.x] = fminf(smin[threadIdx.x], smin[threadIdx.x + s]);
    __syncthreads();
  }
  if (threadIdx.x == 0) block_min[blockIdx.x] = smin[0];
}

// the unstaged form (hsad_act_select): rows read from global memory, any row width; the global minimum comes from min_reduce_kernel
__global__ void act_select_kernel(const float* __restrict__ heads, int ldh, const float* __restrict__ legal,
                                  const float* __restrict__ eps, const float* __restrict__ advmin, int N, int A,
                                  unsigned long long seed, unsigned long long counter, int64_t* __restrict__ a_out,
                                  int64_t* __restrict__ greedy_out) {
  const int m = blockIdx.x * blockDim.x + threadIdx.x;
  if (m >= N) return;
  const as_tail t = as_tail_row(heads + (size_t)m * ldh, legal + (size_t)m * A, A, advmin[0], eps ? eps[m] : 0.f, 0.f, (uint64_t)m, seed,
                                counter, nullptr, 0, false);
  greedy_out[m] = t.greedy;
  a_out[m] = t.act;
}

// ---- the acting tail with everything an actor step needs from the heads in ONE kernel (after adv_min_kernel): the action, the greedy
// action, Q_online(s, a) of the chosen action and, with the target net's heads, Q_target(s, greedy) -- the numbers act_select_kernel +
// min_reduce + q_at_kernel give, in the same arithmetic, from one coalesced pass: a block stages its R rows of heads / legal (and target
// heads) through LDS (row strides 37 / 21 floats are odd: conflict-free), and reduces the per-block minima itself instead of waiting for
// a one-block reduction launch.  eps, qa_out and heads_t (with tq_out) may be NULL: the same for every lane.  One row per lane.
__global__ __launch_bounds__(256) void act_tail_kernel(const float* __restrict__ heads, const float* __restrict__ heads_t, int ldh,
                                                       const float* __restrict__ legal, const float* __restrict__ eps,
                                                       const float* __restrict__ block_min, int nb, int N, int A,
                                                       unsigned long long seed, unsigned long long counter,
                                                       int64_t* __restrict__ a_out, int64_t* __restrict__ greedy_out,
                                                       float* __restrict__ qa_out, float* __restrict__ tq_out, int R) {
  extern __shared__ float s_act[];
  float* s_h = s_act;                    // [R][ldh]   (R <= 256 rows per block: what fits 60 KB of LDS)
  float* s_l = s_act + R * ldh;          // [R][A]
  float* s_t = s_l + R * A;              // [R][ldh]   the target net's heads, when given
  __shared__ float s_red[256];
  const int tid = threadIdx.x, m0 = blockIdx.x * R, rows = min(R, N - m0);
  for (int i = tid; i < rows * ldh; i += 256) s_h[i] = heads[(size_t)m0 * ldh + i];
  for (int i = tid; i < rows * A; i += 256) s_l[i] = legal[(size_t)m0 * A + i];
  if (heads_t)
    for (int i = tid; i < rows * ldh; i += 256) s_t[i] = heads_t[(size_t)m0 * ldh + i];
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
  const float* lg = s_l + tid * A;
  const as_tail t = as_tail_row(s_h + tid * ldh, lg, A, mn, eps ? eps[m] : 0.f, 0.f, (uint64_t)m, seed, counter, nullptr, 0, qa_out != nullptr);
  greedy_out[m] = t.greedy;
  a_out[m] = t.act;
  if (qa_out) qa_out[m] = t.qa;
  if (heads_t) tq_out[m] = as_q_at(s_t + tid * ldh, lg, A, t.greedy);
}

// act_tail_kernel's row (no target heads) at a temperature: as_tail_row WRITTEN OUT in the kernel.  Kept next to the one above for its
// measured speed alone (DESIGN.md section 3c: the same row through as_tail_row costs 0.5 us more of 20.5 at 32,768 rows); launched only
// when temp is given, and held to as_tail_row's restatement and to act_tail_kernel's rows by tests/test_act_sample_kernel_gpu.py.
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
  if (qa_out) qa_out[m] = as_q_from_sum(h, lg, A, act, mean);
}

// Q(s, action) only (the target pass of an actor step: Q_target(s, greedy)): q_head_kernel's value at one action, no [M,A] matrix,
// no minimum
__global__ __launch_bounds__(256) void q_at_kernel(const float* __restrict__ heads, int ldh, const float* __restrict__ legal,
                                                   const int64_t* __restrict__ action, int M, int A, float* __restrict__ qa, int R) {
  extern __shared__ float s_act[];
  float* s_h = s_act;
  float* s_l = s_act + R * ldh;
  const int tid = threadIdx.x, m0 = blockIdx.x * R, rows = min(R, M - m0);
  for (int i = tid; i < rows * ldh; i += 256) s_h[i] = heads[(size_t)m0 * ldh + i];
  for (int i = tid; i < rows * A; i += 256) s_l[i] = legal[(size_t)m0 * A + i];
  __syncthreads();
  if (tid >= rows) return;
  const float* h = s_h + tid * ldh;
  const float* lg = s_l + tid * A;
  qa[m0 + tid] = as_q_at(h, lg, A, (int)action[m0 + tid]);
}

// fp32 h / c [L,N,H] and the bf16 copy of h an acting step carries, zeroed together for the rows whose env terminated.  A wave looks at
// 64 (layer, row) pairs at once (one flag byte per lane, one ballot) and zeroes the few that are set with all its lanes: a step ends
// ~1.5 % of its games, so most waves read 64 bytes and leave.
__global__ __launch_bounds__(256) void zero_state_rows_kernel(float* __restrict__ h, float* __restrict__ c, unsigned* __restrict__ h16,
                                                              const unsigned char* __restrict__ flag, int L, int N, int H,
                                                              int rows_per_flag, int vec) {
  const int lane = threadIdx.x & 63;
  const size_t total = (size_t)L * N;
  const size_t w0 = ((size_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * 64;
  if (w0 >= total) return;
  const size_t wl = w0 + lane;
  const bool set = wl < total && flag[(int)(wl % N) / rows_per_flag] != 0;
  unsigned long long m = __ballot(set);
  while (m) {
    const int b = __ffsll((long long)m) - 1;
    m &= m - 1;
    const size_t w = w0 + b;
    if (vec) {   // H % 8 == 0 and 16-byte aligned bases
      float4* ph = reinterpret_cast<float4*>(h + w * H);
      float4* pc = reinterpret_cast<float4*>(c + w * H);
      for (int i = lane; i < H / 4; i += 64) {
        ph[i] = make_float4(0.f, 0.f, 0.f, 0.f);
        pc[i] = make_float4(0.f, 0.f, 0.f, 0.f);
      }
      if (h16) {
        uint4* p16 = reinterpret_cast<uint4*>(h16 + w * (H / 2));
        for (int i = lane; i < H / 8; i += 64) p16[i] = make_uint4(0u, 0u, 0u, 0u);
      }
    } else {
      for (int i = lane; i < H; i += 64) {
        h[w * H + i] = 0.f;
        c[w * H + i] = 0.f;
      }
      if (h16)
        for (int i = lane; i < H / 2; i += 64) h16[w * (H / 2) + i] = 0u;
    }
  }
}

// R2D2Agent.compute_priority tail (r2d2.py:355-360): |reward + bootstrap * gamma^n * target_qa - online_qa|
__global__ void nstep_priority_kernel(const float* __restrict__ qa, const float* __restrict__ tqa, const float* __restrict__ reward,
                                      const float* __restrict__ bootstrap, float gamma_n, int N, float* __restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < N) out[i] = fabsf(reward[i] + bootstrap[i] * gamma_n * tqa[i] - qa[i]);
}

// zero the rows of fp32 [L, N, H] state whose env terminated (R2D2Actor::postAct, r2d2_actor.h:109-126).  One wave per
// (layer, row): a row whose flag is clear costs one byte read (an actor step ends ~1.5 % of its games).
__global__ __launch_bounds__(256) void zero_rows_kernel(float* __restrict__ x, const unsigned char* __restrict__ flag, int L, int N,
                                                        int H, int rows_per_flag) {
  const size_t w = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);      // (layer, row) index
  if (w >= (size_t)L * N) return;
  const int row = (int)(w % N), lane = threadIdx.x & 63;
  if (!flag[row / rows_per_flag]) return;
  float* p = x + w * H;
  if ((H & 3) == 0 && (((uintptr_t)x) & 15) == 0) {
    for (int i = lane; i < H / 4; i += 64) reinterpret_cast<float4*>(p)[i] = make_float4(0.f, 0.f, 0.f, 0.f);
  } else {
    for (int i = lane; i < H; i += 64) p[i] = 0.f;
  }
}

