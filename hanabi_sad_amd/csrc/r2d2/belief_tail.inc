// belief_tail.inc — the loss of the learned hand belief on the head's logits: per row m = t B + b the negative log-likelihood of the
// true hand under the slot-by-slot model of csrc/hsad_belief_head.h (exact counting belief as base measure, the logits as a tilt), the
// same score at zero logits (the exact belief's), top-1 counters, and the gradient row in bf16.  Specification: include/hsad.h,
// hsad_belief_tail; DESIGN.md section 3g.

// ---------------------------------------------------------------------------------------------------
// One block per sequence b (the cloning tails' shape), eight waves; wave v takes the steps t = v, v + 8, ...  A row is up to five slots
// x 25 types x one hc_count each, int64 work against a table of subset sums.  With the true cards given every slot's pool q_i is
// known up front (teacher forcing), so the slots of a row are independent and its work is spread over the wave:
//   A  lane e (and e + 64, e + 128) fills entry (slot e / 32, subset e % 32) of the slot's table of subset sums in LDS -- hc_tables
//      ONCE per slot, 31 live entries per full row
//   B  lane k (and k + 64) evaluates w[i][t], k = i * 25 + t: one hc_count against the slot's table -> LDS (int64)
//   C  lane i < n walks slot i's 25 types in ascending order (bh_slot_stats, bh_slot_nll, bh_slot_nll0: the header's functions, so the
//      bits are bh_row's) -> mx, 1 / S, the slot's terms and flags in LDS
//   D  lane 0 adds the slots' terms in slot order; every lane stores gradient columns j = lane, lane + 64, ... (bh_prob)
// Each phase ends at a workgroup barrier; the trip count is the same for every thread (rows past T or seq_len skip the work, not the
// barriers).  nll[b] / nll0[b] are sums in ascending t by one thread over per-step terms in LDS, the counters integer sums: the same
// bits run to run, no float atomics.  Nothing is kept in scratch but hc_count's own 32-entry C table.
// ---------------------------------------------------------------------------------------------------
struct BeliefTailArgs {
  const float* logits;
  const int64_t* pool;
  const int32_t *compat, *cards;
  const float *seq_len, *weight;
  int ldz, T, B, Hs;
  float *nll, *nll0;
  int32_t *cards_n, *hits, *hits0, *bad;
  bf16_t* dlogits;      // NULL = no gradient
  int ldo;
};
constexpr int kBeliefTailWaves = 8;
constexpr int kBeliefTailThreads = 64 * kBeliefTailWaves;
struct BeliefWaveLds {
  HcTables tab[HC_MAX_SLOTS];
  int64_t w[HC_MAX_SLOTS * HC_TYPES];
  float mx[HC_MAX_SLOTS], inv[HC_MAX_SLOTS], nll[HC_MAX_SLOTS], nll0[HC_MAX_SLOTS];
  int flags[HC_MAX_SLOTS];      // 1 bad | 2 counted | 4 hit | 8 hit0
  int cnt[4];                   // cards | hits | hits0 | bad of the wave
};
__global__ __launch_bounds__(kBeliefTailThreads) void belief_tail_kernel(BeliefTailArgs p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char s_bt_raw[];
  BeliefWaveLds* s_w = reinterpret_cast<BeliefWaveLds*>(s_bt_raw);
  float* s_x = reinterpret_cast<float*>(s_bt_raw + sizeof(BeliefWaveLds) * kBeliefTailWaves);      // [T] nll of step t
  float* s_x0 = s_x + p.T;                                                                        // [T] nll0 of step t
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, T = p.T, B = p.B, Hs = p.Hs;
  BeliefWaveLds& L = s_w[wave];
  const float len = p.seq_len[b];
  const float scale = p.dlogits ? p.weight[b] / (float)B : 0.f;
  int n_cards = 0, n_hit = 0, n_hit0 = 0, n_bad = 0;      // (lane 0's)
  const int trips = (T + kBeliefTailWaves - 1) / kBeliefTailWaves;
  for (int it = 0; it < trips; ++it) {
    const int t = it * kBeliefTailWaves + wave;
    const bool in_T = t < T;
    const bool valid = in_T && (float)t < len;
    const size_t m = (size_t)(in_T ? t : 0) * B + b;
    const float* z = p.logits + m * p.ldz;
    // the row's knowledge, the same in every lane: pool, masks, true cards, the pool before every slot
    uint64_t q[HC_MAX_SLOTS] = {0, 0, 0, 0, 0};
    uint32_t cm[HC_MAX_SLOTS] = {0, 0, 0, 0, 0};
    int32_t card[HC_MAX_SLOTS] = {-1, -1, -1, -1, -1};
    int n = 0;
    bool row_bad = false;
    if (valid) {
#pragma unroll
      for (int i = 0; i < HC_MAX_SLOTS; ++i)
        if (i < Hs) {
          cm[i] = (uint32_t)p.compat[m * Hs + i] & 0x1ffffffu;
          card[i] = p.cards[m * Hs + i];
        }
      n = bh_occupied(card, HC_MAX_SLOTS);
      row_bad = n < 0;
      if (row_bad) n = 0;
      uint64_t run = (uint64_t)p.pool[m];
#pragma unroll
      for (int i = 0; i < HC_MAX_SLOTS; ++i) {
        q[i] = run;
        if (i < n) {
          if (card[i] < 0 || card[i] >= HC_TYPES) row_bad = true;
          else run -= (uint64_t)1 << (2 * card[i]);
        }
      }
      if (row_bad) n = 0;
    }
    const uint32_t all = hc_all_slots(n);
    // A: the tables of subset sums, one per slot
    for (int e = lane; e < HC_MAX_SLOTS * HC_SUBSETS; e += 64) {
      const int i = e >> 5;
      const uint32_t Bm = (uint32_t)e & 31u, rem = all & ~((2u << i) - 1u);
      if (i < n && Bm != 0u && !(Bm & ~rem)) {
        uint64_t qi = q[0];
#pragma unroll
        for (int k = 1; k < HC_MAX_SLOTS; ++k) qi = i == k ? q[k] : qi;
        const uint32_t am = hc_and_mask(cm, Bm);
        L.tab[i].and_mask[Bm] = am;
        L.tab[i].s[Bm] = hc_weight(qi, am);
      }
    }
    __syncthreads();
    // B: the weights
    for (int k = lane; k < HC_MAX_SLOTS * HC_TYPES; k += 64) {
      const int i = k / HC_TYPES, ty = k - i * HC_TYPES;
      int64_t w = 0;
      if (i < n) {
        uint64_t qi = q[0];
        uint32_t cmi = cm[0];
#pragma unroll
        for (int j = 1; j < HC_MAX_SLOTS; ++j) {
          qi = i == j ? q[j] : qi;
          cmi = i == j ? cm[j] : cmi;
        }
        w = bh_weight(L.tab[i].and_mask, L.tab[i].s, qi, cmi, all & ~((2u << i) - 1u), ty);
      }
      L.w[k] = w;
    }
    __syncthreads();
    // C: one lane per slot
    if (lane < HC_MAX_SLOTS) {
      const int i = lane;
      int fl = 0;
      float mx = 0.f, inv = 0.f, a = 0.f, a0 = 0.f;
      if (i < n) {
        const float* zi = z + i * HC_TYPES;
        const int64_t* wi = L.w + i * HC_TYPES;
        const bh_slot_stats_t st = bh_slot_stats(zi, wi);
        int c = card[0];
#pragma unroll
        for (int j = 1; j < HC_MAX_SLOTS; ++j) c = i == j ? card[j] : c;
        if (!st.finite || st.nfeas == 0 || wi[c] == 0) {
          fl = 1;
        } else {
          mx = st.mx;
          inv = 1.f / st.S;
          a = bh_slot_nll(st, zi[c], wi[c]);
          a0 = bh_slot_nll0(st, wi[c]);
          if (st.nfeas >= 2) fl = 2 | (st.best == c ? 4 : 0) | (st.best0 == c ? 8 : 0);
        }
      }
      L.mx[i] = mx;
      L.inv[i] = inv;
      L.nll[i] = a;
      L.nll0[i] = a0;
      L.flags[i] = fl;
    }
    __syncthreads();
    // D: the row
    if (valid) {
      for (int i = 0; i < n; ++i) row_bad = row_bad || (L.flags[i] & 1);
    }
    if (lane == 0 && in_T) {
      float a = 0.f, a0 = 0.f;
      if (valid && !row_bad)
        for (int i = 0; i < n; ++i) {
          a += L.nll[i];
          a0 += L.nll0[i];
          const int fl = L.flags[i];
          n_cards += (fl >> 1) & 1;
          n_hit += (fl >> 2) & 1;
          n_hit0 += (fl >> 3) & 1;
        }
      n_bad += valid && row_bad;
      s_x[t] = a;
      s_x0[t] = a0;
    }
    if (p.dlogits && in_T) {
      bf16_t* o = p.dlogits + m * p.ldo;
      const bool grad = valid && !row_bad;
      for (int j = lane; j < p.ldo; j += 64) {
        float v = 0.f;
        if (grad && j < n * HC_TYPES) {
          const int i = j / HC_TYPES, ty = j - i * HC_TYPES;
          const int64_t w = L.w[j];
          int c = card[0];
#pragma unroll
          for (int k = 1; k < HC_MAX_SLOTS; ++k) c = i == k ? card[k] : c;
          if (w != 0) v = scale * (bh_prob(z[j], w, L.mx[i], L.inv[i]) - (ty == c ? 1.f : 0.f));
        }
        o[j] = f2bf(v);
      }
    }
    // (the next trip's phase A writes the tables only; L.w and the slot terms are rewritten behind its barriers)
  }
  if (lane == 0) {
    L.cnt[0] = n_cards;
    L.cnt[1] = n_hit;
    L.cnt[2] = n_hit0;
    L.cnt[3] = n_bad;
  }
  __syncthreads();
  if (tid == 0) {
    float total = 0.f, total0 = 0.f;
    for (int t = 0; t < T; ++t) {      // ascending t (the cloning tails' order)
      total += s_x[t];
      total0 += s_x0[t];
    }
    p.nll[b] = total;
    p.nll0[b] = total0;
    int c[4] = {0, 0, 0, 0};
    for (int w = 0; w < kBeliefTailWaves; ++w)
      for (int k = 0; k < 4; ++k) c[k] += s_w[w].cnt[k];
    p.cards_n[b] = c[0];
    p.hits[b] = c[1];
    p.hits0[b] = c[2];
    p.bad[b] = c[3];
  }
}
